// Sphere area lights: Sphere::area / sample / sample_with_ref_point / pdf_with_ref_point (src/shapes/sphere.rs:361-504) and DiffuseAreaLight::sample_li /
// pdf_li / power over that shape (src/lights/diffuse.rs:64-103), operation by operation in f32, uncontracted like the rest of the library.
// Compiled into the kernels that carry the sphere-light need only (SL: k_sphere_light, k_ld_fixed_sl, k_ld_contrib_sl); every other kernel keeps its code.
// The reference point is an InteractionCommon's p, p_error and n (SlRef): the inside test runs on pnt3_offset_ray_origin of the three, and a bare point
// (SpatialLightDistribution::compute_distribution, lightdistrib.rs:169-260) is the same function with p_error = n = 0.
#pragma once
#include "dev_sphere.h"

namespace rspt {

struct SlRef {
    f3 p, p_err, n;
};

RDEV float sphere_area(const rspt_sphere& s) { return s.phi_max * s.radius * (s.z_max - s.z_min); }   // sphere.rs:361-363

// transform.rs:709-769 transform_point_with_abs_error
RDEV f3 xf_point_abs_err(const float* m, f3 p, f3 pe, f3* err) {
    const float g3 = gamma_n(3);
    const float xp = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
    const float yp = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
    const float zp = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
    const float wp = m[12] * p.x + m[13] * p.y + m[14] * p.z + m[15];
    *err = f3{(g3 + 1.0f) * (fabsf(m[0]) * pe.x + fabsf(m[1]) * pe.y + fabsf(m[2]) * pe.z) + g3 * (fabsf(m[0] * p.x) + fabsf(m[1] * p.y) + fabsf(m[2] * p.z) + fabsf(m[3])),
              (g3 + 1.0f) * (fabsf(m[4]) * pe.x + fabsf(m[5]) * pe.y + fabsf(m[6]) * pe.z) + g3 * (fabsf(m[4] * p.x) + fabsf(m[5] * p.y) + fabsf(m[6] * p.z) + fabsf(m[7])),
              (g3 + 1.0f) * (fabsf(m[8]) * pe.x + fabsf(m[9]) * pe.y + fabsf(m[10]) * pe.z) + g3 * (fabsf(m[8] * p.x) + fabsf(m[9] * p.y) + fabsf(m[10] * p.z) + fabsf(m[11]))};
    if (wp == 1.0f) return f3{xp, yp, zp};
    const float inv = 1.0f / wp;
    return f3{inv * xp, inv * yp, inv * zp};
}

// Sphere::sample (sphere.rs:364-390): the WHOLE sphere is sampled, clipped or not
RDEVN LightSample sphere_sample(const rspt_sphere& s, f2 u, float* pdf) {
    // uniform_sample_sphere (sampling.rs:327-336)
    const float z = 1.0f - 2.0f * u.x;
    const float r = sqrtf(fmaxf(0.0f, 1.0f - z * z));
    const float phi = 2.0f * RSPT_PI * u.y;
    const f3 dir{r * rspt_cosf(phi), r * rspt_sinf(phi), z};
    f3 p_obj = f3{0.0f, 0.0f, 0.0f} + dir * s.radius;
    LightSample it;
    it.n = normalize(xf_normal(s.world_to_object, p_obj));
    if (s.reverse_orientation) it.n = it.n * -1.0f;
    p_obj = p_obj * (s.radius / len(p_obj - f3{0.0f, 0.0f, 0.0f}));
    const f3 p_obj_err = vabs(p_obj) * gamma_n(5);
    it.p = xf_point_abs_err(s.object_to_world, p_obj, p_obj_err, &it.p_err);
    *pdf = 1.0f / sphere_area(s);
    return it;
}

// the test both ref-point functions open with (sphere.rs:397-401, :469-477)
RDEV bool sphere_ref_inside(const rspt_sphere& s, const SlRef& ref, f3* p_center) {
    *p_center = xf_point(s.object_to_world, f3{0.0f, 0.0f, 0.0f});
    const f3 p_origin = offset_ray_origin(ref.p, ref.p_err, ref.n, *p_center - ref.p);
    return dist2(p_origin, *p_center) <= s.radius * s.radius;
}

// Sphere::sample_with_ref_point (sphere.rs:391-467)
RDEVN LightSample sphere_sample_ref(const rspt_sphere& s, const SlRef& ref, f2 u, float* pdf) {
    f3 p_center;
    if (sphere_ref_inside(s, ref, &p_center)) {
        const LightSample intr = sphere_sample(s, u, pdf);
        f3 wi = intr.p - ref.p;
        if (len2(wi) == 0.0f) *pdf = 0.0f;
        else {
            wi = normalize(wi);
            *pdf *= dist2(ref.p, intr.p) / absdot(intr.n, -wi);
        }
        if (__builtin_isinf(*pdf)) *pdf = 0.0f;
        return intr;
    }
    const f3 wc = normalize(p_center - ref.p);
    f3 wc_x, wc_y;
    coordinate_system(wc, &wc_x, &wc_y);
    const float sin_theta_max2 = s.radius * s.radius / dist2(ref.p, p_center);
    const float cos_theta_max = sqrtf(fmaxf(0.0f, 1.0f - sin_theta_max2));
    const float cos_theta = (1.0f - u.x) + u.x * cos_theta_max;
    const float sin_theta = sqrtf(fmaxf(0.0f, 1.0f - cos_theta * cos_theta));
    const float phi = u.y * 2.0f * RSPT_PI;
    const float dc = len(ref.p - p_center);
    const float ds = dc * cos_theta - sqrtf(fmaxf(0.0f, s.radius * s.radius - dc * dc * sin_theta * sin_theta));
    const float cos_alpha = (dc * dc + s.radius * s.radius - ds * ds) / (2.0f * dc * s.radius);
    const float sin_alpha = sqrtf(fmaxf(0.0f, 1.0f - cos_alpha * cos_alpha));
    // spherical_direction_vec3 (geometry.rs:1570-1579)
    const f3 n_world = (-wc_x) * (sin_alpha * rspt_cosf(phi)) + (-wc_y) * (sin_alpha * rspt_sinf(phi)) + (-wc) * cos_alpha;
    LightSample it;
    it.p = p_center + n_world * s.radius;
    it.p_err = vabs(it.p) * gamma_n(5);
    it.n = n_world;
    if (s.reverse_orientation) it.n = it.n * -1.0f;
    *pdf = 1.0f / (2.0f * RSPT_PI * (1.0f - cos_theta_max));
    return it;
}

// Sphere::pdf_with_ref_point (sphere.rs:468-504).  Inside: Sphere::intersect on iref.spawn_ray(wi) (interaction.rs:64-80), t_max = infinity
RDEVN float sphere_pdf_ref(const rspt_sphere& s, const SlRef& ref, f3 wi) {
    f3 p_center;
    if (sphere_ref_inside(s, ref, &p_center)) {
        SphereHit sh;
        if (!sphere_hit(s, offset_ray_origin(ref.p, ref.p_err, ref.n, wi), wi, RSPT_INF, &sh)) return 0.0f;
        float pdf = dist2(ref.p, sh.p) / (absdot(sh.n, -wi) * sphere_area(s));
        if (__builtin_isinf(pdf)) pdf = 0.0f;
        return pdf;
    }
    const float sin_theta_max2 = s.radius * s.radius / dist2(ref.p, p_center);
    const float cos_theta_max = sqrtf(fmaxf(0.0f, 1.0f - sin_theta_max2));
    return 1.0f / (2.0f * RSPT_PI * (1.0f - cos_theta_max));   // uniform_cone_pdf (sampling.rs:369-371)
}

// DiffuseAreaLight::sample_li over a sphere (diffuse.rs:64-84): l() is taken with the SAMPLED normal
RDEVN rgb sphere_light_sample_li(const rspt_sphere& s, const rspt_light& lt, const SlRef& ref, f2 u, f3* wi, float* pdf, LightSample* ls) {
    *ls = sphere_sample_ref(s, ref, u, pdf);
    if (*pdf == 0.0f || len2(ls->p - ref.p) == 0.0f) { *pdf = 0.0f; return mkrgb(0.0f); }
    *wi = normalize(ls->p - ref.p);
    return light_l(lt, ls->n, -*wi);
}
// DiffuseAreaLight::power (diffuse.rs:85-93) with area = shape.area()
RDEV rgb sphere_light_power(const rspt_sphere& s, const rspt_light& lt) {
    const float factor = lt.two_sided ? 2.0f : 1.0f;
    return ldrgb(lt.L) * factor * sphere_area(s) * RSPT_PI;
}

}  // namespace rspt
