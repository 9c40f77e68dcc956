// Analytic spheres (ABI 23): Sphere::intersect / intersect_p (src/shapes/sphere.rs:103-360) over EFloat (src/core/efloat.rs) and
// Transform::transform_ray_with_error (src/core/transform.rs:793-814), operation by operation in f32 (the discriminant in f64), uncontracted
// like the rest of the library.  The traversal kernels call sphere_test (t only); the stage hook RSPT_LIBM_SPHERE and the shade / texture /
// AO stages (kernels.h sphere_fill) call sphere_hit, which also builds the SurfaceInteraction and transforms it to world space (transform.rs:815-860).
//
// Device layout: a scene with spheres keeps them behind its 48-byte triangle records in the same buffer (SceneDev::tris), 176 bytes each
// (rspt_sphere + 8 bytes of padding), so that no kernel signature and no SceneDev field changes.  A sphere primitive's record carries the
// sphere index in t0.x and MF_SPHERE in the flags word.
#pragma once
#include "dev_scene.h"
#include "../../include/rspt.h"

namespace rspt {

struct SphereDev {   // 176 B = 11 float4
    rspt_sphere s;
    uint32_t pad[2];
};
static_assert(sizeof(rspt_sphere) == 168, "rspt_sphere layout");
static_assert(sizeof(SphereDev) == 176, "SphereDev layout");
#define RSPT_SPHERE_F4 11u   // float4 slots per sphere behind the triangle records

// efloat.rs:48-200
struct EF {
    float v, lo, hi;
};
RDEV EF ef_new(float v, float err) { return err == 0.0f ? EF{v, v, v} : EF{v, next_down(v - err), next_up(v + err)}; }
RDEV EF ef_add(EF a, EF b) { return EF{a.v + b.v, next_down(a.lo + b.lo), next_up(a.hi + b.hi)}; }
RDEV EF ef_sub(EF a, EF b) { return EF{a.v - b.v, next_down(a.lo - b.hi), next_up(a.hi - b.lo)}; }
RDEV EF ef_mul(EF a, EF b) {
    const float p0 = a.lo * b.lo, p1 = a.hi * b.lo, p2 = a.lo * b.hi, p3 = a.hi * b.hi;
    return EF{a.v * b.v, next_down(fminf(fminf(p0, p1), fminf(p2, p3))), next_up(fmaxf(fmaxf(p0, p1), fmaxf(p2, p3)))};
}
RDEV EF ef_mulf(EF a, float f) { return ef_mul(EF{f, f, f}, a); }   // Mul<f32>: EFloat::new(rhs, 0.0) * self
RDEV EF ef_div(EF a, EF b) {
    if (b.lo < 0.0f && b.hi > 0.0f) return EF{a.v / b.v, -RSPT_INF, RSPT_INF};
    const float d0 = a.lo / b.lo, d1 = a.hi / b.lo, d2 = a.lo / b.hi, d3 = a.hi / b.hi;
    return EF{a.v / b.v, next_down(fminf(fminf(d0, d1), fminf(d2, d3))), next_up(fmaxf(fmaxf(d0, d1), fmaxf(d2, d3)))};
}
// efloat.rs:16-37
RDEV bool quadratic_ef(EF a, EF b, EF c, EF* t0, EF* t1) {
    const double discrim = (double)b.v * (double)b.v - 4.0 * (double)a.v * (double)c.v;
    if (discrim < 0.0) return false;
    const double root = sqrt(discrim);
    const EF frd = ef_new((float)root, RSPT_MACHINE_EPS * (float)root);
    const EF q = b.v < 0.0f ? ef_mulf(ef_sub(b, frd), -0.5f) : ef_mulf(ef_add(b, frd), -0.5f);
    EF x0 = ef_div(q, a), x1 = ef_div(c, q);
    if (x0.v > x1.v) { const EF t = x0; x0 = x1; x1 = t; }
    *t0 = x0; *t1 = x1;
    return true;
}

// xf_point_err / xf_vector (dev_math.h) and xf_normal (dev_scene.h) are transform.rs:662-708, :518-537 as the instances use them
// transform.rs:793-814: the origin is pushed along d to the edge of its error box; t_max is kept
RDEV void xf_ray_err(const float* m, f3 o, f3 d, f3* oo, f3* od, f3* o_err, f3* d_err) {
    f3 p = xf_point_err(m, o, o_err);
    const float g3 = gamma_n(3);
    *d_err = f3{g3 * (fabsf(m[0] * d.x) + fabsf(m[1] * d.y) + fabsf(m[2] * d.z)), g3 * (fabsf(m[4] * d.x) + fabsf(m[5] * d.y) + fabsf(m[6] * d.z)),
                g3 * (fabsf(m[8] * d.x) + fabsf(m[9] * d.y) + fabsf(m[10] * d.z))};
    const f3 v = xf_vector(m, d);
    const float l2 = len2(v);
    if (l2 > 0.0f) {
        const float dt = dot(vabs(v), *o_err) / l2;
        p = p + v * dt;
    }
    *oo = p; *od = v;
}

// the refined hit point and phi of sphere.rs:162-172 for a candidate t
RDEV void sphere_point(const rspt_sphere& s, f3 o, f3 d, float t, f3* p_out, float* phi_out) {
    f3 p = o + d * t;
    p = p * (s.radius / len(p));
    if (p.x == 0.0f && p.y == 0.0f) p.x = 1e-5f * s.radius;
    float phi = rspt_atan2f(p.y, p.x);
    if (phi < 0.0f) phi += 2.0f * RSPT_PI;
    *p_out = p; *phi_out = phi;
}
RDEV bool sphere_clipped(const rspt_sphere& s, f3 p, float phi) {
    return (s.z_min > -s.radius && p.z < s.z_min) || (s.z_max < s.radius && p.z > s.z_max) || phi > s.phi_max;
}

// The first half of Sphere::intersect / intersect_p (they are the same up to the interaction): the object-space ray, t_shape_hit, p_hit, phi.
// t_max is the world ray's (transform_ray_with_error keeps it).
RDEVN bool sphere_core(const rspt_sphere& s, f3 wo, f3 wd, float t_max, EF* t_hit, f3* p_hit, float* phi_hit, f3* od_out) {
    f3 o, d, oe, de;
    xf_ray_err(s.world_to_object, wo, wd, &o, &d, &oe, &de);
    const EF ox = ef_new(o.x, oe.x), oy = ef_new(o.y, oe.y), oz = ef_new(o.z, oe.z);
    const EF dx = ef_new(d.x, de.x), dy = ef_new(d.y, de.y), dz = ef_new(d.z, de.z);
    const EF a = ef_add(ef_add(ef_mul(dx, dx), ef_mul(dy, dy)), ef_mul(dz, dz));
    const EF b = ef_mulf(ef_add(ef_add(ef_mul(dx, ox), ef_mul(dy, oy)), ef_mul(dz, oz)), 2.0f);
    const EF r = ef_new(s.radius, 0.0f);
    const EF c = ef_sub(ef_add(ef_add(ef_mul(ox, ox), ef_mul(oy, oy)), ef_mul(oz, oz)), ef_mul(r, r));
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
    sphere_point(s, o, d, th.v, &p, &phi);
    if (sphere_clipped(s, p, phi)) {
        if (th.v == t1.v) return false;   // EFloat's PartialEq compares v
        if (t1.hi > t_max) return false;
        th = t1;
        sphere_point(s, o, d, th.v, &p, &phi);
        if (sphere_clipped(s, p, phi)) return false;
    }
    *t_hit = th; *p_hit = p; *phi_hit = phi;
    if (od_out) *od_out = d;
    return true;
}

// what the traversal needs: hit or not, and t_shape_hit.v (primitive.rs:150-156 makes it the ray's t_max)
RDEV bool sphere_test(const rspt_sphere& s, f3 o, f3 d, float t_max, float* t_out) {
    EF th;
    f3 p;
    float phi;
    if (!sphere_core(s, o, d, t_max, &th, &p, &phi, nullptr)) return false;
    *t_out = th.v;
    return true;
}

// Sphere::intersect's interaction (sphere.rs:196-267) after object_to_world.transform_surface_interaction (transform.rs:815-860).  The shape
// handed to SurfaceInteraction::new is None, so n is never flipped.  The shading frame starts as the geometric one and faceforward of a normal
// against itself keeps it: it is returned as computed, for the hook to show.
struct SphereHit {
    float t;
    f3 p, p_error, n;
    float u, v;
    f3 dpdu, dpdv, dndu, dndv;
    f3 sn, sdpdu, sdpdv, sdndu, sdndv;
};
RDEVN bool sphere_hit(const rspt_sphere& s, f3 wo, f3 wd, float t_max, SphereHit* h) {
    EF th;
    f3 ph;
    float phi;
    if (!sphere_core(s, wo, wd, t_max, &th, &ph, &phi, nullptr)) return false;
    const float u = phi / s.phi_max;
    const float theta = rspt_acosf(clampf(ph.z / s.radius, -1.0f, 1.0f));
    const float dth = s.theta_max - s.theta_min;
    const float v = (theta - s.theta_min) / dth;
    const float z_radius = sqrtf(ph.x * ph.x + ph.y * ph.y);
    const float inv_z_radius = 1.0f / z_radius;
    const float cos_phi = ph.x * inv_z_radius, sin_phi = ph.y * inv_z_radius;
    const f3 dpdu{-s.phi_max * ph.y, s.phi_max * ph.x, 0.0f};
    const f3 dpdv = f3{ph.z * cos_phi, ph.z * sin_phi, -s.radius * rspt_sinf(theta)} * dth;
    const f3 d2_p_duu = (f3{ph.x, ph.y, 0.0f} * -s.phi_max) * s.phi_max;
    const f3 d2_p_duv = ((f3{-sin_phi, cos_phi, 0.0f} * dth) * ph.z) * s.phi_max;
    const f3 d2_p_dvv = (f3{ph.x, ph.y, ph.z} * -dth) * dth;
    const float ec = dot(dpdu, dpdu), fc = dot(dpdu, dpdv), gc = dot(dpdv, dpdv);
    const f3 nc = normalize(cross(dpdu, dpdv));
    const float el = dot(nc, d2_p_duu), fl = dot(nc, d2_p_duv), gl = dot(nc, d2_p_dvv);
    const float inv_egf2 = 1.0f / (ec * gc - fc * fc);
    const f3 dndu = (dpdu * (fl * fc - el * gc)) * inv_egf2 + (dpdv * (el * fc - fl * ec)) * inv_egf2;
    const f3 dndv = (dpdu * (gl * fc - fl * gc)) * inv_egf2 + (dpdv * (fl * fc - gl * ec)) * inv_egf2;
    const f3 p_err = vabs(ph) * gamma_n(5);
    const f3 n = normalize(cross(dpdu, dpdv));   // SurfaceInteraction::new (interaction.rs:259-280)
    // transform_surface_interaction: p with transform_point_with_abs_error (transform.rs:709-769)
    const float* m = s.object_to_world;
    const float* mi = s.world_to_object;
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
    h->t = th.v;
    h->n = normalize(xf_normal(mi, n));
    h->u = u; h->v = v;
    h->dpdu = xf_vector(m, dpdu); h->dpdv = xf_vector(m, dpdv);
    h->dndu = xf_normal(mi, dndu); h->dndv = xf_normal(mi, dndv);
    h->sn = faceforward(normalize(xf_normal(mi, n)), h->n);
    h->sdpdu = xf_vector(m, dpdu); h->sdpdv = xf_vector(m, dpdv);
    h->sdndu = xf_normal(mi, dndu); h->sdndv = xf_normal(mi, dndv);
    return true;
}

}  // namespace rspt
