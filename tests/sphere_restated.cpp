// Test helper (compiled by tests/test_gpu_spheres.py with g++ into a temporary directory): a hand restatement of Sphere::intersect /
// intersect_p (src/shapes/sphere.rs:103-360), EFloat and quadratic_efloat (src/core/efloat.rs), Transform::transform_ray_with_error and
// transform_surface_interaction (src/core/transform.rs:662-860), written from the reference's text, and a walk of an rspt_bvh_node array in
// BVHAccel::intersect / intersect_p's order (bvh.rs:401-514) over those spheres and the oracle's watertight triangle test.
// f32 throughout with the host libm (acosf, atan2f, sinf), the discriminant in f64; build with -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "orc_render.hpp"

namespace {

float bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t ubits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
// pbrt.rs:61-91
float next_float_up(float v) {
    if (std::isinf(v) && v > 0.0f) return v;
    const float nv = v == -0.0f ? 0.0f : v;
    uint32_t ui = ubits(nv);
    if (nv >= 0.0f) ui += 1; else ui -= 1;
    return bits(ui);
}
float next_float_down(float v) {
    if (std::isinf(v) && v < 0.0f) return v;
    const float nv = v == 0.0f ? -0.0f : v;
    uint32_t ui = ubits(nv);
    if (nv > 0.0f) ui -= 1; else ui += 1;
    return bits(ui);
}
const float MACHINE_EPSILON = 1.1920929e-7f * 0.5f;
float gamma(int n) { return ((float)n * MACHINE_EPSILON) / (1.0f - (float)n * MACHINE_EPSILON); }
float fmin_(float a, float b) { return std::fmin(a, b); }   // f32::min / max: the other operand when one is NaN
float fmax_(float a, float b) { return std::fmax(a, b); }

struct EFloat {
    float v, low, high;
};
EFloat ef(float v, float err) { return err == 0.0f ? EFloat{v, v, v} : EFloat{v, next_float_down(v - err), next_float_up(v + err)}; }
EFloat operator+(EFloat a, EFloat b) { return EFloat{a.v + b.v, next_float_down(a.low + b.low), next_float_up(a.high + b.high)}; }
EFloat operator-(EFloat a, EFloat b) { return EFloat{a.v - b.v, next_float_down(a.low - b.high), next_float_up(a.high - b.low)}; }
EFloat operator*(EFloat a, EFloat b) {
    const float p[4] = {a.low * b.low, a.high * b.low, a.low * b.high, a.high * b.high};
    return EFloat{a.v * b.v, next_float_down(fmin_(fmin_(p[0], p[1]), fmin_(p[2], p[3]))), next_float_up(fmax_(fmax_(p[0], p[1]), fmax_(p[2], p[3])))};
}
EFloat operator*(EFloat a, float f) { return ef(f, 0.0f) * a; }
EFloat operator/(EFloat a, EFloat b) {
    const float q[4] = {a.low / b.low, a.high / b.low, a.low / b.high, a.high / b.high};
    if (b.low < 0.0f && b.high > 0.0f) return EFloat{a.v / b.v, -INFINITY, INFINITY};
    return EFloat{a.v / b.v, next_float_down(fmin_(fmin_(q[0], q[1]), fmin_(q[2], q[3]))), next_float_up(fmax_(fmax_(q[0], q[1]), fmax_(q[2], q[3])))};
}
bool quadratic(EFloat a, EFloat b, EFloat c, EFloat* t0, EFloat* t1) {
    const double discrim = (double)b.v * (double)b.v - 4.0 * (double)a.v * (double)c.v;
    if (discrim < 0.0) return false;
    const double root_discrim = std::sqrt(discrim);
    const EFloat frd = ef((float)root_discrim, MACHINE_EPSILON * (float)root_discrim);
    const EFloat q = b.v < 0.0f ? (b - frd) * -0.5f : (b + frd) * -0.5f;
    *t0 = q / a;
    *t1 = c / q;
    if (t0->v > t1->v) { EFloat t = *t0; *t0 = *t1; *t1 = t; }
    return true;
}

struct V { float x, y, z; };
V add(V a, V b) { return V{a.x + b.x, a.y + b.y, a.z + b.z}; }
V mul(V a, float s) { return V{a.x * s, a.y * s, a.z * s}; }
float vdot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V vcross(V a, V b) {   // geometry.rs:680-692: f64 products
    const double ax = a.x, ay = a.y, az = a.z, bx = b.x, by = b.y, bz = b.z;
    return V{(float)(ay * bz - az * by), (float)(az * bx - ax * bz), (float)(ax * by - ay * bx)};
}
V vnormalize(V a) { const float l = std::sqrt(vdot(a, a)); const float inv = 1.0f / l; return V{a.x * inv, a.y * inv, a.z * inv}; }
V vabs(V a) { return V{std::fabs(a.x), std::fabs(a.y), std::fabs(a.z)}; }

V point_with_error(const float* m, V p, V* err) {
    const float xp = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
    const float yp = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
    const float zp = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
    const float wp = m[12] * p.x + m[13] * p.y + m[14] * p.z + m[15];
    const float xs = std::fabs(m[0] * p.x) + std::fabs(m[1] * p.y) + std::fabs(m[2] * p.z) + std::fabs(m[3]);
    const float ys = std::fabs(m[4] * p.x) + std::fabs(m[5] * p.y) + std::fabs(m[6] * p.z) + std::fabs(m[7]);
    const float zs = std::fabs(m[8] * p.x) + std::fabs(m[9] * p.y) + std::fabs(m[10] * p.z) + std::fabs(m[11]);
    *err = V{xs * gamma(3), ys * gamma(3), zs * gamma(3)};
    if (wp == 1.0f) return V{xp, yp, zp};
    const float inv = 1.0f / wp;
    return V{inv * xp, inv * yp, inv * zp};
}
V vector_with_error(const float* m, V v, V* err) {
    const float g = gamma(3);
    *err = V{g * (std::fabs(m[0] * v.x) + std::fabs(m[1] * v.y) + std::fabs(m[2] * v.z)), g * (std::fabs(m[4] * v.x) + std::fabs(m[5] * v.y) + std::fabs(m[6] * v.z)),
             g * (std::fabs(m[8] * v.x) + std::fabs(m[9] * v.y) + std::fabs(m[10] * v.z))};
    return V{m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z, m[8] * v.x + m[9] * v.y + m[10] * v.z};
}
V xvec(const float* m, V v) { return V{m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z, m[8] * v.x + m[9] * v.y + m[10] * v.z}; }
V xnrm(const float* mi, V n) { return V{mi[0] * n.x + mi[4] * n.y + mi[8] * n.z, mi[1] * n.x + mi[5] * n.y + mi[9] * n.z, mi[2] * n.x + mi[6] * n.y + mi[10] * n.z}; }

struct Hit {
    float t;
    V p, p_error, n;
    float u, v;
    V dpdu, dpdv, dndu, dndv, sn, sdpdu, sdpdv, sdndu, sdndv;
};

// Sphere::intersect (full = true) / intersect_p (full = false)
bool sphere_intersect(const rspt_sphere& s, V wo, V wd, float t_max, bool full, Hit* h) {
    V o_err, d_err;
    V o = point_with_error(s.world_to_object, wo, &o_err);
    const V d = vector_with_error(s.world_to_object, wd, &d_err);
    const float ls = vdot(d, d);
    if (ls > 0.0f) {
        const float dt = vdot(vabs(d), o_err) / ls;
        o = add(o, mul(d, dt));
    }
    const EFloat ox = ef(o.x, o_err.x), oy = ef(o.y, o_err.y), oz = ef(o.z, o_err.z);
    const EFloat dx = ef(d.x, d_err.x), dy = ef(d.y, d_err.y), dz = ef(d.z, d_err.z);
    const EFloat a = dx * dx + dy * dy + dz * dz;
    const EFloat b = (dx * ox + dy * oy + dz * oz) * 2.0f;
    const EFloat c = ox * ox + oy * oy + oz * oz - ef(s.radius, 0.0f) * ef(s.radius, 0.0f);
    EFloat t0, t1;
    if (!quadratic(a, b, c, &t0, &t1)) return false;
    if (t0.high > t_max || t1.low <= 0.0f) return false;
    EFloat ts = t0;
    if (ts.low <= 0.0f) {
        ts = t1;
        if (ts.high > t_max) return false;
    }
    auto position = [&](float t, V* p, float* phi) {
        V q = add(o, mul(d, t));
        const float dist = std::sqrt(vdot(q, q));
        q = mul(q, s.radius / dist);
        if (q.x == 0.0f && q.y == 0.0f) q.x = 1e-5f * s.radius;
        float f = std::atan2(q.y, q.x);
        if (f < 0.0f) f += 2.0f * (float)M_PI;
        *p = q; *phi = f;
    };
    auto clipped = [&](V p, float phi) { return (s.z_min > -s.radius && p.z < s.z_min) || (s.z_max < s.radius && p.z > s.z_max) || phi > s.phi_max; };
    V ph;
    float phi;
    position(ts.v, &ph, &phi);
    if (clipped(ph, phi)) {
        if (ts.v == t1.v) return false;
        if (t1.high > t_max) return false;
        ts = t1;
        position(ts.v, &ph, &phi);
        if (clipped(ph, phi)) return false;
    }
    h->t = ts.v;
    if (!full) return true;
    const float u = phi / s.phi_max;
    float zr = ph.z / s.radius;
    zr = zr < -1.0f ? -1.0f : (zr > 1.0f ? 1.0f : zr);
    const float theta = std::acos(zr);
    const float v = (theta - s.theta_min) / (s.theta_max - s.theta_min);
    const float z_radius = std::sqrt(ph.x * ph.x + ph.y * ph.y);
    const float inv_z_radius = 1.0f / z_radius;
    const float cos_phi = ph.x * inv_z_radius, sin_phi = ph.y * inv_z_radius;
    const V dpdu{-s.phi_max * ph.y, s.phi_max * ph.x, 0.0f};
    const V dpdv = mul(V{ph.z * cos_phi, ph.z * sin_phi, -s.radius * std::sin(theta)}, s.theta_max - s.theta_min);
    const V d2duu = mul(mul(V{ph.x, ph.y, 0.0f}, -s.phi_max), s.phi_max);
    const V d2duv = mul(mul(mul(V{-sin_phi, cos_phi, 0.0f}, s.theta_max - s.theta_min), ph.z), s.phi_max);
    const V d2dvv = mul(mul(V{ph.x, ph.y, ph.z}, -(s.theta_max - s.theta_min)), s.theta_max - s.theta_min);
    const float E = vdot(dpdu, dpdu), F = vdot(dpdu, dpdv), G = vdot(dpdv, dpdv);
    const V nc = vnormalize(vcross(dpdu, dpdv));
    const float e = vdot(nc, d2duu), f = vdot(nc, d2duv), g = vdot(nc, d2dvv);
    const float inv_egf2 = 1.0f / (E * G - F * F);
    const V dndu = add(mul(mul(dpdu, f * F - e * G), inv_egf2), mul(mul(dpdv, e * F - f * E), inv_egf2));
    const V dndv = add(mul(mul(dpdu, g * F - f * G), inv_egf2), mul(mul(dpdv, f * F - g * E), inv_egf2));
    const V perr = mul(vabs(ph), gamma(5));
    const V n = vnormalize(vcross(dpdu, dpdv));   // SurfaceInteraction::new with shape None: no flip
    // object_to_world.transform_surface_interaction
    const float* m = s.object_to_world;
    const float* mi = s.world_to_object;
    const float g3 = gamma(3);
    const float xp = m[0] * ph.x + m[1] * ph.y + m[2] * ph.z + m[3];
    const float yp = m[4] * ph.x + m[5] * ph.y + m[6] * ph.z + m[7];
    const float zp = m[8] * ph.x + m[9] * ph.y + m[10] * ph.z + m[11];
    const float wp = m[12] * ph.x + m[13] * ph.y + m[14] * ph.z + m[15];
    float ae[3];
    for (int r = 0; r < 3; r++) {
        const float* row = m + 4 * r;
        ae[r] = (g3 + 1.0f) * (std::fabs(row[0]) * perr.x + std::fabs(row[1]) * perr.y + std::fabs(row[2]) * perr.z) +
                g3 * (std::fabs(row[0] * ph.x) + std::fabs(row[1] * ph.y) + std::fabs(row[2] * ph.z) + std::fabs(row[3]));
    }
    h->p_error = V{ae[0], ae[1], ae[2]};
    if (wp == 1.0f) h->p = V{xp, yp, zp};
    else { const float inv = 1.0f / wp; h->p = V{inv * xp, inv * yp, inv * zp}; }
    h->n = vnormalize(xnrm(mi, n));
    h->u = u; h->v = v;
    h->dpdu = xvec(m, dpdu); h->dpdv = xvec(m, dpdv); h->dndu = xnrm(mi, dndu); h->dndv = xnrm(mi, dndv);
    V sn = vnormalize(xnrm(mi, n));
    if (vdot(sn, h->n) < 0.0f) sn = V{-sn.x, -sn.y, -sn.z};   // nrm_faceforward_nrm
    h->sn = sn; h->sdpdu = h->dpdu; h->sdpdv = h->dpdv; h->sdndu = h->dndu; h->sdndv = h->dndv;
    return true;
}

}  // namespace

extern "C" {
// the layout of RSPT_LIBM_SPHERE (include/rspt.h): 64 floats in, 64 out per element
void sph_hook(const float* x, uint64_t n, float* out) {
    for (uint64_t i = 0; i < n; i++) {
        rspt_sphere s;
        std::memcpy(&s, x + 64 * i, sizeof s);
        const float* q = x + 64 * i + 42;
        float* r = out + 64 * i;
        for (int k = 0; k < 64; k++) r[k] = 0.0f;
        Hit h;
        if (sphere_intersect(s, V{q[0], q[1], q[2]}, V{q[3], q[4], q[5]}, q[6], true, &h)) {
            const V v[13] = {h.p, h.p_error, h.n, V{h.u, h.v, 0.0f}, h.dpdu, h.dpdv, h.dndu, h.dndv, h.sn, h.sdpdu, h.sdpdv, h.sdndu, h.sdndv};
            r[0] = 1.0f; r[1] = h.t;
            int k = 2;
            for (int j = 0; j < 13; j++) { r[k++] = v[j].x; r[k++] = v[j].y; if (j != 3) r[k++] = v[j].z; }
        }
        Hit hp;
        r[43] = sphere_intersect(s, V{q[0], q[1], q[2]}, V{q[3], q[4], q[5]}, q[6], false, &hp) ? 1.0f : 0.0f;
    }
}

// BVHAccel::intersect (any = 0) / intersect_p (any = 1) over triangles (the oracle's watertight test) and spheres.  Meshes with an alpha mask
// are given a constant-0 mask by the tests: no candidate on them is ever a hit (triangle.rs:313-330, :593-655).
void sph_walk(const rspt_scene_desc* desc, const rspt_ray* rays, uint64_t n, int any, rspt_hit* out) {
    orc::Scene sc{};
    sc.d = *desc;
    for (uint64_t i = 0; i < n; i++) {
        orc::Ray ray{};
        ray.o = orc::V3{rays[i].o[0], rays[i].o[1], rays[i].o[2]};
        ray.d = orc::V3{rays[i].d[0], rays[i].d[1], rays[i].d[2]};
        ray.t_max = rays[i].t_max;
        rspt_hit hit{0xffffffffu, 0.0f, 0.0f, 0.0f, 0.0f};
        if (desc->n_nodes) {
            const orc::V3 inv{1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z};
            const uint8_t neg[3] = {(uint8_t)(inv.x < 0.0f), (uint8_t)(inv.y < 0.0f), (uint8_t)(inv.z < 0.0f)};
            uint32_t to_visit = 0, cur = 0, stack[64];
            bool done = false;
            for (;;) {
                const rspt_bvh_node& node = desc->nodes[cur];
                if (orc::Scene::box_hit(node, ray, inv, neg)) {
                    if (node.n_prims > 0) {
                        for (uint32_t k = 0; k < node.n_prims && !done; k++) {
                            const uint32_t pi = (uint32_t)node.offset + k;
                            const rspt_prim& pr = desc->prims[pi];
                            float t = 0.0f, b[3] = {0.0f, 0.0f, 0.0f};
                            bool h;
                            if (pr.mesh == RSPT_MESH_SPHERE) {
                                Hit sh;
                                h = sphere_intersect(desc->spheres[pr.v[0]], V{ray.o.x, ray.o.y, ray.o.z}, V{ray.d.x, ray.d.y, ray.d.z}, ray.t_max, false, &sh);
                                t = sh.t;
                            } else {
                                h = sc.tri_hit_test(pr, ray, &t, b) && !(desc->meshes[pr.mesh].alpha_tex || desc->meshes[pr.mesh].shadow_alpha_tex);
                            }
                            if (!h) continue;
                            if (any) { hit.prim = 0; done = true; break; }
                            ray.t_max = t;
                            hit.prim = pi; hit.t = t; hit.b0 = b[0]; hit.b1 = b[1]; hit.b2 = b[2];
                        }
                        if (done || to_visit == 0) break;
                        cur = stack[--to_visit];
                    } else if (neg[node.axis]) { stack[to_visit++] = cur + 1; cur = (uint32_t)node.offset; }
                    else { stack[to_visit++] = (uint32_t)node.offset; cur = cur + 1; }
                } else {
                    if (to_visit == 0) break;
                    cur = stack[--to_visit];
                }
            }
        }
        out[i] = hit;
    }
}
}
