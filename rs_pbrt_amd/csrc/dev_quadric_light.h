// Disk and cylinder area lights: Disk::area / sample / sample_with_ref_point / pdf_with_ref_point (src/shapes/disk.rs:207-280), the same four of Cylinder
// (src/shapes/cylinder.rs:331-415) and DiffuseAreaLight::sample_li / pdf_li / power over them (src/lights/diffuse.rs:64-103), operation by operation in f32,
// uncontracted like the rest of the library.  What the reference does is reproduced as written, not repaired: Disk::sample ignores inner_radius and phi_max
// (points of the cut-away part come back, with the pdf of the true area), both areas are object-space figures, the cylinder's normal is taken before the
// reprojection.  Compiled into the kernels that carry the quadric-light need only (QL: k_quadric_light, k_ld_fixed_ql, k_ld_contrib_ql, k_shade_ql); every
// other kernel keeps its code.  The reference point is an SlRef as for sphere lights; a bare point is the same function with p_error = n = 0.
#pragma once
#include "dev_quadric.h"
#include "dev_sphere_light.h"

namespace rspt {

RDEV float disk_area(const rspt_disk& s) { return s.phi_max * 0.5f * (s.radius * s.radius - s.inner_radius * s.inner_radius); }   // disk.rs:207-211
RDEV float cylinder_area(const rspt_cylinder& s) { return (s.z_max - s.z_min) * s.radius * s.phi_max; }                           // cylinder.rs:331-333

// Disk::sample (disk.rs:212-239): the FULL disk of `radius`, whatever inner_radius and phi_max say; the object-space error is zero
RDEVN LightSample disk_sample(const rspt_disk& s, f2 u, float* pdf) {
    const f2 pd = concentric_disk(u);
    const f3 p_obj{pd.x * s.radius, pd.y * s.radius, s.height};
    LightSample it;
    it.n = normalize(xf_normal(s.world_to_object, f3{0.0f, 0.0f, 1.0f}));
    if (s.reverse_orientation) it.n = it.n * -1.0f;
    it.p = xf_point_abs_err(s.object_to_world, p_obj, f3{0.0f, 0.0f, 0.0f}, &it.p_err);
    *pdf = 1.0f / disk_area(s);
    return it;
}
// Cylinder::sample (cylinder.rs:334-374): the normal from the point before the reprojection
RDEVN LightSample cylinder_sample(const rspt_cylinder& s, f2 u, float* pdf) {
    const float z = lerpf(u.x, s.z_min, s.z_max);
    const float phi = u.y * s.phi_max;
    f3 p_obj{s.radius * rspt_cosf(phi), s.radius * rspt_sinf(phi), z};
    LightSample it;
    it.n = normalize(xf_normal(s.world_to_object, f3{p_obj.x, p_obj.y, 0.0f}));
    if (s.reverse_orientation) it.n = it.n * -1.0f;
    const float hit_rad = sqrtf(p_obj.x * p_obj.x + p_obj.y * p_obj.y);
    p_obj.x *= s.radius / hit_rad;
    p_obj.y *= s.radius / hit_rad;
    const f3 p_obj_err = vabs(f3{p_obj.x, p_obj.y, 0.0f}) * gamma_n(3);
    it.p = xf_point_abs_err(s.object_to_world, p_obj, p_obj_err, &it.p_err);
    *pdf = 1.0f / cylinder_area(s);
    return it;
}
// the tail both shapes' sample_with_ref_point share (disk.rs:246-259, cylinder.rs:381-394): area measure to solid angle
RDEV void quadric_pdf_to_solid_angle(const LightSample& intr, const SlRef& ref, float* pdf) {
    f3 wi = intr.p - ref.p;
    if (len2(wi) == 0.0f) *pdf = 0.0f;
    else {
        wi = normalize(wi);
        *pdf *= dist2(ref.p, intr.p) / absdot(intr.n, -wi);
        if (__builtin_isinf(*pdf)) *pdf = 0.0f;
    }
}
RDEVN LightSample disk_sample_ref(const rspt_disk& s, const SlRef& ref, f2 u, float* pdf) {
    const LightSample intr = disk_sample(s, u, pdf);
    quadric_pdf_to_solid_angle(intr, ref, pdf);
    return intr;
}
RDEVN LightSample cylinder_sample_ref(const rspt_cylinder& s, const SlRef& ref, f2 u, float* pdf) {
    const LightSample intr = cylinder_sample(s, u, pdf);
    quadric_pdf_to_solid_angle(intr, ref, pdf);
    return intr;
}
// pdf_with_ref_point (disk.rs:261-280, cylinder.rs:396-415): the shape's own intersect on iref.spawn_ray(wi) (interaction.rs:64-80), t_max = infinity;
// disk_hit / cylinder_hit honour inner_radius, phi_max and the z clip, so a direction toward a cut-away point has pdf 0
RDEVN float disk_pdf_ref(const rspt_disk& s, const SlRef& ref, f3 wi) {
    SphereHit sh;
    if (!disk_hit(s, offset_ray_origin(ref.p, ref.p_err, ref.n, wi), wi, RSPT_INF, &sh)) return 0.0f;
    float pdf = dist2(ref.p, sh.p) / (absdot(sh.n, -wi) * disk_area(s));
    if (__builtin_isinf(pdf)) pdf = 0.0f;
    return pdf;
}
RDEVN float cylinder_pdf_ref(const rspt_cylinder& s, const SlRef& ref, f3 wi) {
    SphereHit sh;
    if (!cylinder_hit(s, offset_ray_origin(ref.p, ref.p_err, ref.n, wi), wi, RSPT_INF, &sh)) return 0.0f;
    float pdf = dist2(ref.p, sh.p) / (absdot(sh.n, -wi) * cylinder_area(s));
    if (__builtin_isinf(pdf)) pdf = 0.0f;
    return pdf;
}

// ---- over a slot of any kind (QuadricDev): what the kernels call.  A sphere slot goes to dev_sphere_light.h's functions unchanged. ----
RDEV float quadric_area(const QuadricDev& q) {
    if (q.kind == QK_DISK) return disk_area(q.d);
    if (q.kind == QK_CYLINDER) return cylinder_area(q.c);
    return sphere_area(q.s);
}
RDEV LightSample quadric_sample(const QuadricDev& q, f2 u, float* pdf) {
    if (q.kind == QK_DISK) return disk_sample(q.d, u, pdf);
    if (q.kind == QK_CYLINDER) return cylinder_sample(q.c, u, pdf);
    return sphere_sample(q.s, u, pdf);
}
RDEV LightSample quadric_sample_ref(const QuadricDev& q, const SlRef& ref, f2 u, float* pdf) {
    if (q.kind == QK_DISK) return disk_sample_ref(q.d, ref, u, pdf);
    if (q.kind == QK_CYLINDER) return cylinder_sample_ref(q.c, ref, u, pdf);
    return sphere_sample_ref(q.s, ref, u, pdf);
}
RDEV float quadric_pdf_ref(const QuadricDev& q, const SlRef& ref, f3 wi) {
    if (q.kind == QK_DISK) return disk_pdf_ref(q.d, ref, wi);
    if (q.kind == QK_CYLINDER) return cylinder_pdf_ref(q.c, ref, wi);
    return sphere_pdf_ref(q.s, ref, wi);
}
// DiffuseAreaLight::sample_li over the slot's shape (diffuse.rs:64-84): l() is taken with the SAMPLED normal
RDEVN rgb quadric_light_sample_li(const QuadricDev& q, const rspt_light& lt, const SlRef& ref, f2 u, f3* wi, float* pdf, LightSample* ls) {
    *ls = quadric_sample_ref(q, ref, u, pdf);
    if (*pdf == 0.0f || len2(ls->p - ref.p) == 0.0f) { *pdf = 0.0f; return mkrgb(0.0f); }
    *wi = normalize(ls->p - ref.p);
    return light_l(lt, ls->n, -*wi);
}
// DiffuseAreaLight::power (diffuse.rs:85-93) with area = shape.area(): the object-space figure, the transform's scale never enters
RDEV rgb quadric_light_power(const QuadricDev& q, const rspt_light& lt) {
    const float factor = lt.two_sided ? 2.0f : 1.0f;
    return ldrgb(lt.L) * factor * quadric_area(q) * RSPT_PI;
}

}  // namespace rspt
