// Test helper (compiled by tests/test_quadric_render_host.py and tests/test_gpu_quadric_render.py with g++ into a temporary directory): the
// restatement of PathIntegrator::li, uniform_sample_one_light / estimate_direct and AOIntegrator::li of tests/sphere_render_restated.cpp over
// a scene view whose BVH walk (bvh.rs:401-514) tests all four primitive kinds: triangles by the oracle's own primitive tests, spheres by
// tests/sphere_restated.cpp, disks and cylinders by tests/quadric_restated.cpp.  The li functions below are that file's, line for line, bound
// to this file's intersect / intersect_p (they are not templates over the walk, so they are stated again); tests/test_quadric_render_host.py
// holds them to the oracle's li on triangle scenes and to tests/sphere_render_restated.cpp on sphere scenes, bit for bit.
// f32 throughout with the host libm; build with -ffp-contract=off.
#include "sphere_render_restated.cpp"
#define QUADRIC_RESTATED_HAVE_SPHERE
#include "quadric_restated.cpp"

namespace orc {
namespace quadr {

// GeometricPrimitive::intersect (primitive.rs:150-186) over a Disk or a Cylinder: sphr::sphere_interaction reads nothing of its record but the two
// matrices and the media, which lead and end all three records alike
template <class Shape>
void quadric_interaction(const Shape& s, const Ray& ray, const ::Hit& h, uint32_t pi, Interaction* it) {
    rspt_sphere as{};
    std::memcpy(as.object_to_world, s.object_to_world, sizeof as.object_to_world);
    std::memcpy(as.world_to_object, s.world_to_object, sizeof as.world_to_object);
    as.medium_inside = s.medium_inside; as.medium_outside = s.medium_outside;
    sphr::sphere_interaction(as, ray, h, pi, it);
}

// Scene::intersect -> BVHAccel::intersect (scene.rs:55-66, bvh.rs:401-462): every primitive of a leaf is tested, a hit shrinks ray.t_max
bool intersect(const Scene& sc, const Ray& ray, Interaction* isect, Counters* c) {
    if (c) c->rays_closest++;
    if (sc.d.n_nodes == 0) return false;
    bool hit = false;
    const V3 inv_dir{1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z};
    const uint8_t neg[3] = {(uint8_t)(inv_dir.x < 0.0f), (uint8_t)(inv_dir.y < 0.0f), (uint8_t)(inv_dir.z < 0.0f)};
    uint32_t to_visit = 0, cur = 0, stack[64];
    for (;;) {
        const rspt_bvh_node& node = sc.d.nodes[cur];
        if (Scene::box_hit(node, ray, inv_dir, neg)) {
            if (node.n_prims > 0) {
                for (uint32_t i = 0; i < node.n_prims; i++) {
                    const uint32_t pi = (uint32_t)node.offset + i;
                    const rspt_prim& pr = sc.d.prims[pi];
                    const ::V o{ray.o.x, ray.o.y, ray.o.z}, d{ray.d.x, ray.d.y, ray.d.z};
                    ::Hit h;
                    if (pr.mesh == RSPT_MESH_SPHERE) {
                        const rspt_sphere& s = sc.d.spheres[pr.v[0]];
                        if (sphere_intersect(s, o, d, ray.t_max, true, &h)) {
                            ray.t_max = h.t;   // primitive.rs:155
                            sphr::sphere_interaction(s, ray, h, pi, isect);
                            hit = true;
                        }
                    } else if (pr.mesh == RSPT_MESH_DISK) {
                        const rspt_disk& s = sc.d.disks[pr.v[0]];
                        if (disk_intersect(s, o, d, ray.t_max, true, &h)) {
                            ray.t_max = h.t;
                            quadric_interaction(s, ray, h, pi, isect);
                            hit = true;
                        }
                    } else if (pr.mesh == RSPT_MESH_CYLINDER) {
                        const rspt_cylinder& s = sc.d.cylinders[pr.v[0]];
                        if (cylinder_intersect(s, o, d, ray.t_max, true, &h)) {
                            ray.t_max = h.t;
                            quadric_interaction(s, ray, h, pi, isect);
                            hit = true;
                        }
                    } else if (sc.prim_intersect(pi, ray, isect, nullptr, nullptr, nullptr))
                        hit = true;
                }
                if (to_visit == 0) break;
                cur = stack[--to_visit];
            } else if (neg[node.axis]) { stack[to_visit++] = cur + 1; cur = (uint32_t)node.offset; }
            else { stack[to_visit++] = (uint32_t)node.offset; cur = cur + 1; }
        } else {
            if (to_visit == 0) break;
            cur = stack[--to_visit];
        }
    }
    return hit;
}
// Scene::intersect_p -> BVHAccel::intersect_p (bvh.rs:463-514): the first primitive that reports a hit ends the walk
bool intersect_p(const Scene& sc, const Ray& ray, Counters* c) {
    if (c) c->rays_any++;
    if (sc.d.n_nodes == 0) return false;
    const V3 inv_dir{1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z};
    const uint8_t neg[3] = {(uint8_t)(inv_dir.x < 0.0f), (uint8_t)(inv_dir.y < 0.0f), (uint8_t)(inv_dir.z < 0.0f)};
    uint32_t to_visit = 0, cur = 0, stack[64];
    for (;;) {
        const rspt_bvh_node& node = sc.d.nodes[cur];
        if (Scene::box_hit(node, ray, inv_dir, neg)) {
            if (node.n_prims > 0) {
                for (uint32_t i = 0; i < node.n_prims; i++) {
                    const uint32_t pi = (uint32_t)node.offset + i;
                    const rspt_prim& pr = sc.d.prims[pi];
                    const ::V o{ray.o.x, ray.o.y, ray.o.z}, d{ray.d.x, ray.d.y, ray.d.z};
                    ::Hit h;
                    if (pr.mesh == RSPT_MESH_SPHERE) {
                        if (sphere_intersect(sc.d.spheres[pr.v[0]], o, d, ray.t_max, false, &h)) return true;
                    } else if (pr.mesh == RSPT_MESH_DISK) {
                        if (disk_intersect(sc.d.disks[pr.v[0]], o, d, ray.t_max, false, &h)) return true;
                    } else if (pr.mesh == RSPT_MESH_CYLINDER) {
                        if (cylinder_intersect(sc.d.cylinders[pr.v[0]], o, d, ray.t_max, false, &h)) return true;
                    } else if (sc.prim_intersect_p(pi, ray, nullptr))
                        return true;
                }
                if (to_visit == 0) break;
                cur = stack[--to_visit];
            } else if (neg[node.axis]) { stack[to_visit++] = cur + 1; cur = (uint32_t)node.offset; }
            else { stack[to_visit++] = (uint32_t)node.offset; cur = cur + 1; }
        } else {
            if (to_visit == 0) break;
            cur = stack[--to_visit];
        }
    }
    return false;
}

// integrator.rs:407-570
Spec estimate_direct(RenderCtx& cx, const Interaction& it, const Bsdf& bsdf, P2 u_scattering, uint32_t light_num, P2 u_light, Counters* c) {
    const Scene& sc = *cx.scene;
    const rspt_light& light = sc.d.lights[light_num];
    const uint8_t bsdf_flags = BSDF_ALL & ~BSDF_SPECULAR;   // :416-420
    Spec ld(0.0f);
    V3 wi{0, 0, 0};
    Float light_pdf = 0.0f, scattering_pdf = 0.0f;
    Interaction light_intr;
    Spec li = light_sample_li(sc, light, it, u_light, &wi, &light_pdf, &light_intr);   // :424-432
    if (light_pdf > 0.0f && !li.is_black()) {
        Spec f = bsdf.f(it.wo, wi, bsdf_flags) * Spec(abs_dot(wi, it.sh_n));   // :437-443
        scattering_pdf = bsdf.pdf(it.wo, wi, bsdf_flags);
        if (!f.is_black()) {
            if (intersect_p(sc, it.spawn_ray_to(light_intr), c)) li = Spec(0.0f);   // VisibilityTester::unoccluded (light.rs:199-206), :456-466
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
                light_pdf = light.kind == RSPT_LIGHT_INFINITE ? infinite_pdf_li(sc, light, wi) : sc.tri_pdf_ref(sc.d.prims[light.prim], it, wi);
                if (light_pdf == 0.0f) return ld;
                weight = power_heuristic(1, scattering_pdf, 1, light_pdf);
            }
            const Ray ray = it.spawn_ray(wi);   // :530-548
            Spec li2;
            Interaction light_isect;
            if (intersect(sc, ray, &light_isect, c)) {
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
Spec uniform_sample_one_light(RenderCtx& cx, const Interaction& it, const Bsdf& bsdf, Sampler& sampler, const Distribution1D& distrib, Counters* c) {
    if (cx.scene->d.n_lights == 0) return Spec();
    Float pdf = 0.0f;
    const size_t light_num = distrib.sample_discrete(sampler.get_1d(), &pdf);
    if (pdf == 0.0f) return Spec();
    const P2 u_light = sampler.get_2d();
    const P2 u_scattering = sampler.get_2d();
    return quadr::estimate_direct(cx, it, bsdf, u_scattering, (uint32_t)light_num, u_light, c) / pdf;
}

// path.rs:59-282
Spec path_li(RenderCtx& cx, const Ray& r, Sampler& sampler, Counters* c) {
    const Scene& sc = *cx.scene;
    Spec l, beta(1.0f);
    Ray ray = r;
    bool specular_bounce = false;
    uint32_t bounces = 0;
    Float eta_scale = 1.0f;
    for (;;) {
        Interaction isect;
        if (intersect(sc, ray, &isect, c)) {   // :77-81
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
            const Distribution1D* distrib = sc.d.n_lights ? light_lookup(cx, isect.p) : nullptr;   // :118
            if (sc.d.n_lights && bsdf.num_components(BSDF_ALL & ~BSDF_SPECULAR) > 0)   // :120-139
                l = l + beta * quadr::uniform_sample_one_light(cx, isect, bsdf, sampler, *distrib, c);
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

// ao.rs:50-96
Spec ao_li(RenderCtx& cx, const Ray& ray, Sampler& sampler, Counters* c) {
    const Scene& sc = *cx.scene;
    const rspt_render_desc& rd = *cx.rd;
    Spec l;
    Interaction isect;
    if (intersect(sc, ray, &isect, c)) {
        const V3 n = faceforward(isect.n, -ray.d);   // :66-69
        const V3 s = normalize(isect.dpdu);
        const V3 t = cross(isect.n, s);
        const int32_t ns = (int32_t)rd.ao_n_samples;
        size_t which = 0;
        uint64_t first = 0;
        const bool have = sampler.get_2d_array(ns, &which, &first);   // :75
        for (int32_t k = 0; have && k < ns; k++) {
            const P2 u = sampler.get_2d_sample(which, first + (uint64_t)k);
            V3 wi;
            Float pdf;
            if (rd.ao_cos_sample) { wi = cosine_sample_hemisphere(u); pdf = std::fabs(wi.z) * INV_PI; }   // :80-86
            else { wi = uniform_sample_hemisphere(u); pdf = INV_2_PI; }
            wi = V3{s.x * wi.x + t.x * wi.y + n.x * wi.z, s.y * wi.x + t.y * wi.y + n.y * wi.z, s.z * wi.x + t.z * wi.y + n.z * wi.z};   // :88-92
            if (pdf != 0.0f && !intersect_p(sc, isect.spawn_ray(wi), c)) l = l + Spec(dot(wi, n) / (pdf * (Float)ns));   // :93-95
        }
    }
    return l;
}

}  // namespace quadr
}  // namespace orc

extern "C" {
// orc::render with li replaced by the restatement above; film_xyzw (npix, 4) and li_rgb (npix * spp * 3) as orc_render fills them
int qr_render(const rspt_scene_desc* sd, const rspt_render_desc* rd, int num_threads, float* film_xyzw, float* li_rgb) {
    if (!sd || !rd) return -1;
    orc::g_li_override = orc::quadr::path_li;
    orc::g_ao_li_override = orc::quadr::ao_li;
    orc::Scene sc{*sd};
    orc::RenderOut out;
    orc::render(sc, *rd, num_threads, film_xyzw, li_rgb, &out);
    orc::g_li_override = nullptr;
    orc::g_ao_li_override = nullptr;
    return 0;
}
}
