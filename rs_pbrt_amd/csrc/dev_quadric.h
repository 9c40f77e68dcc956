// Disks and cylinders (ABI 27): Disk::intersect / intersect_p (src/shapes/disk.rs:92-197) and Cylinder::intersect / intersect_p
// (src/shapes/cylinder.rs:95-320), operation by operation in f32, uncontracted, over the pieces dev_sphere.h built for spheres: EF,
// quadratic_ef, xf_ray_err.  The tail that turns the object-space interaction into the world one (transform_surface_interaction,
// transform.rs:815-860) is stated again here as quadric_to_world instead of being cut out of sphere_hit, so that the sphere kernels keep
// their code and their register figures.
//
// Device layout: a scene with a disk or a cylinder keeps ALL its quadrics — spheres first, then disks, then cylinders — behind its triangle
// records in the 176-byte slots spheres take (SphereDev, RSPT_SPHERE_F4), the shape's kind in the first of the slot's two padding words
// (0 = sphere: a sphere-only scene's records are those of ABI 23).  A quadric primitive's record carries the slot index in t0.x and MF_SPHERE
// in the flags word, so every stage that tells such a record from a triangle does so as before; only the instantiations such a scene takes
// (trace_w4.h QUAD, dev_bsdf.h shade_quad, kernels.h k_texture_quad / k_ao_spawn_quad) read the kind.
#pragma once
#include "dev_sphere.h"

namespace rspt {

enum : uint32_t { QK_SPHERE = 0, QK_DISK = 1, QK_CYLINDER = 2 };
struct QuadricDev {   // 176 B = 11 float4, the slot of a SphereDev
    union {
        rspt_sphere s;
        rspt_disk d;
        rspt_cylinder c;
    };
    uint32_t kind, pad;
};
static_assert(sizeof(rspt_disk) == 160 && sizeof(rspt_cylinder) == 160, "rspt_disk / rspt_cylinder layout");
static_assert(sizeof(QuadricDev) == sizeof(SphereDev) && offsetof(QuadricDev, kind) == offsetof(SphereDev, pad), "QuadricDev shares the sphere slot");

// transform_surface_interaction (transform.rs:815-860) of an interaction SurfaceInteraction::new made with shape None (interaction.rs:259-280):
// p by transform_point_with_abs_error (transform.rs:709-769), n never flipped, the shading frame a copy of the geometric one (sphere_hit's tail)
RDEV void quadric_to_world(const float* m, const float* mi, float t, f3 ph, f3 p_err, float u, float v, f3 dpdu, f3 dpdv, f3 dndu, f3 dndv, SphereHit* h) {
    const f3 n = normalize(cross(dpdu, dpdv));
    const float g3 = gamma_n(3);
    const float xp = m[0] * ph.x + m[1] * ph.y + m[2] * ph.z + m[3];
    const float yp = m[4] * ph.x + m[5] * ph.y + m[6] * ph.z + m[7];
    const float zp = m[8] * ph.x + m[9] * ph.y + m[10] * ph.z + m[11];
    const float wp = m[12] * ph.x + m[13] * ph.y + m[14] * ph.z + m[15];
    h->p_error = f3{(g3 + 1.0f) * (fabsf(m[0]) * p_err.x + fabsf(m[1]) * p_err.y + fabsf(m[2]) * p_err.z) +
                        g3 * (fabsf(m[0] * ph.x) + fabsf(m[1] * ph.y) + fabsf(m[2] * ph.z) + fabsf(m[3])),
                    (g3 + 1.0f) * (fabsf(m[4]) * p_err.x + fabsf(m[5]) * p_err.y + fabsf(m[6]) * p_err.z) +
                        g3 * (fabsf(m[4] * ph.x) + fabsf(m[5] * ph.y) + fabsf(m[6] * ph.z) + fabsf(m[7])),
                    (g3 + 1.0f) * (fabsf(m[8]) * p_err.x + fabsf(m[9]) * p_err.y + fabsf(m[10]) * p_err.z) +
                        g3 * (fabsf(m[8] * ph.x) + fabsf(m[9] * ph.y) + fabsf(m[10] * ph.z) + fabsf(m[11]))};
    if (wp == 1.0f) h->p = f3{xp, yp, zp};
    else { const float inv = 1.0f / wp; h->p = f3{inv * xp, inv * yp, inv * zp}; }
    h->t = t;
    h->n = normalize(xf_normal(mi, n));
    h->u = u; h->v = v;
    h->dpdu = xf_vector(m, dpdu); h->dpdv = xf_vector(m, dpdv);
    h->dndu = xf_normal(mi, dndu); h->dndv = xf_normal(mi, dndv);
    h->sn = faceforward(normalize(xf_normal(mi, n)), h->n);
    h->sdpdu = xf_vector(m, dpdu); h->sdpdv = xf_vector(m, dpdv);
    h->sdndu = xf_normal(mi, dndu); h->sdndv = xf_normal(mi, dndv);
}

// ---- Disk (disk.rs:92-197): a plane test in plain f32, no EFloat.  intersect and intersect_p are the same up to the interaction. ----
// One candidate t, and t_max only ever rejects it (t >= t_max: note the >=), so a hit the traversal accepted under a smaller t_max comes out
// of the same branches with the same p under the ray's own (kernels.h quadric_fill).
RDEVN bool disk_core(const rspt_disk& s, f3 wo, f3 wd, float t_max, float* t_hit, f3* p_hit, float* phi_hit) {
    f3 o, d, oe, de;
    xf_ray_err(s.world_to_object, wo, wd, &o, &d, &oe, &de);
    if (d.z == 0.0f) return false;
    const float t = (s.height - o.z) / d.z;
    if (t <= 0.0f || t >= t_max) return false;
    const f3 p = o + d * t;
    const float dist2 = p.x * p.x + p.y * p.y;
    if (dist2 > s.radius * s.radius || dist2 < s.inner_radius * s.inner_radius) return false;
    float phi = rspt_atan2f(p.y, p.x);
    if (phi < 0.0f) phi += 2.0f * RSPT_PI;
    if (phi > s.phi_max) return false;
    *t_hit = t; *p_hit = p; *phi_hit = phi;
    return true;
}
RDEV bool disk_test(const rspt_disk& s, f3 o, f3 d, float t_max, float* t_out) {
    f3 p;
    float phi;
    return disk_core(s, o, d, t_max, t_out, &p, &phi);
}
RDEVN bool disk_hit(const rspt_disk& s, f3 wo, f3 wd, float t_max, SphereHit* h) {
    float t, phi;
    f3 ph;
    if (!disk_core(s, wo, wd, t_max, &t, &ph, &phi)) return false;
    const float dist2 = ph.x * ph.x + ph.y * ph.y;
    const float u = phi / s.phi_max;
    const float r_hit = sqrtf(dist2);
    const float one_minus_v = (r_hit - s.inner_radius) / (s.radius - s.inner_radius);
    const float v = 1.0f - one_minus_v;
    const f3 dpdu{-s.phi_max * ph.y, s.phi_max * ph.x, 0.0f};
    const f3 dpdv = (f3{ph.x, ph.y, 0.0f} * (s.inner_radius - s.radius)) * (1.0f / r_hit);   // Vector3f / f32 multiplies by the reciprocal (geometry.rs:1271-1279)
    const f3 zero{0.0f, 0.0f, 0.0f};
    ph.z = s.height;   // the refinement comes after dist2 and phi (disk.rs:144)
    quadric_to_world(s.object_to_world, s.world_to_object, t, ph, zero, u, v, dpdu, dpdv, zero, zero, h);
    return true;
}

// ---- Cylinder (cylinder.rs:95-320): Sphere::intersect with a quadratic over x and y only; z carries no EFloat ----
RDEV void cylinder_point(const rspt_cylinder& s, f3 o, f3 d, float t, f3* p_out, float* phi_out) {
    f3 p = o + d * t;
    const float hit_rad = sqrtf(p.x * p.x + p.y * p.y);
    p.x *= s.radius / hit_rad;
    p.y *= s.radius / hit_rad;
    float phi = rspt_atan2f(p.y, p.x);
    if (phi < 0.0f) phi += 2.0f * RSPT_PI;
    *p_out = p; *phi_out = phi;
}
RDEV bool cylinder_clipped(const rspt_cylinder& s, f3 p, float phi) { return p.z < s.z_min || p.z > s.z_max || phi > s.phi_max; }
RDEVN bool cylinder_core(const rspt_cylinder& s, f3 wo, f3 wd, float t_max, EF* t_hit, f3* p_hit, float* phi_hit) {
    f3 o, d, oe, de;
    xf_ray_err(s.world_to_object, wo, wd, &o, &d, &oe, &de);
    const EF ox = ef_new(o.x, oe.x), oy = ef_new(o.y, oe.y);
    const EF dx = ef_new(d.x, de.x), dy = ef_new(d.y, de.y);
    const EF a = ef_add(ef_mul(dx, dx), ef_mul(dy, dy));
    const EF b = ef_mulf(ef_add(ef_mul(dx, ox), ef_mul(dy, oy)), 2.0f);
    const EF r = ef_new(s.radius, 0.0f);
    const EF c = ef_sub(ef_add(ef_mul(ox, ox), ef_mul(oy, oy)), ef_mul(r, r));
    EF t0, t1;
    if (!quadratic_ef(a, b, c, &t0, &t1)) return false;
    if (t0.hi > t_max || t1.lo <= 0.0f) return false;
    EF th = t0;
    if (th.lo <= 0.0f) {
        th = t1;
        if (th.hi > t_max) return false;
    }
    f3 p;
    float phi;
    cylinder_point(s, o, d, th.v, &p, &phi);
    if (cylinder_clipped(s, p, phi)) {
        if (th.v == t1.v) return false;   // EFloat's PartialEq compares v
        th = t1;
        if (t1.hi > t_max) return false;
        cylinder_point(s, o, d, th.v, &p, &phi);
        if (cylinder_clipped(s, p, phi)) return false;
    }
    *t_hit = th; *p_hit = p; *phi_hit = phi;
    return true;
}
RDEV bool cylinder_test(const rspt_cylinder& s, f3 o, f3 d, float t_max, float* t_out) {
    EF th;
    f3 p;
    float phi;
    if (!cylinder_core(s, o, d, t_max, &th, &p, &phi)) return false;
    *t_out = th.v;
    return true;
}
RDEVN bool cylinder_hit(const rspt_cylinder& s, f3 wo, f3 wd, float t_max, SphereHit* h) {
    EF th;
    f3 ph;
    float phi;
    if (!cylinder_core(s, wo, wd, t_max, &th, &ph, &phi)) return false;
    const float u = phi / s.phi_max;
    const float v = (ph.z - s.z_min) / (s.z_max - s.z_min);
    const f3 dpdu{-s.phi_max * ph.y, s.phi_max * ph.x, 0.0f};
    const f3 dpdv{0.0f, 0.0f, s.z_max - s.z_min};
    const f3 d2_p_duu = (f3{ph.x, ph.y, 0.0f} * -s.phi_max) * s.phi_max;
    const f3 d2_p_duv{0.0f, 0.0f, 0.0f}, d2_p_dvv{0.0f, 0.0f, 0.0f};
    const float ec = dot(dpdu, dpdu), fc = dot(dpdu, dpdv), gc = dot(dpdv, dpdv);
    const f3 nc = normalize(cross(dpdu, dpdv));
    const float el = dot(nc, d2_p_duu), fl = dot(nc, d2_p_duv), gl = dot(nc, d2_p_dvv);
    const float inv_egf2 = 1.0f / (ec * gc - fc * fc);
    const f3 dndu = (dpdu * (fl * fc - el * gc)) * inv_egf2 + (dpdv * (el * fc - fl * ec)) * inv_egf2;
    const f3 dndv = (dpdu * (gl * fc - fl * gc)) * inv_egf2 + (dpdv * (fl * fc - gl * ec)) * inv_egf2;
    const f3 p_err = vabs(f3{ph.x, ph.y, 0.0f}) * gamma_n(3);
    quadric_to_world(s.object_to_world, s.world_to_object, th.v, ph, p_err, u, v, dpdu, dpdv, dndu, dndv, h);
    return true;
}

// what the traversal and the stages call on a record of any kind
RDEV bool quadric_test(const QuadricDev& q, f3 o, f3 d, float t_max, float* t_out) {
    if (q.kind == QK_DISK) return disk_test(q.d, o, d, t_max, t_out);
    if (q.kind == QK_CYLINDER) return cylinder_test(q.c, o, d, t_max, t_out);
    return sphere_test(q.s, o, d, t_max, t_out);
}
RDEV bool quadric_hit(const QuadricDev& q, f3 o, f3 d, float t_max, SphereHit* h) {
    if (q.kind == QK_DISK) return disk_hit(q.d, o, d, t_max, h);
    if (q.kind == QK_CYLINDER) return cylinder_hit(q.c, o, d, t_max, h);
    return sphere_hit(q.s, o, d, t_max, h);
}

}  // namespace rspt
