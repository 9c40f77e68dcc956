// Test helper (compiled by tests/test_quadric_host.py and tests/test_gpu_quadrics.py with g++ into a temporary directory): a hand restatement
// of Disk::intersect / intersect_p (src/shapes/disk.rs:92-197) and Cylinder::intersect / intersect_p (src/shapes/cylinder.rs:95-320) with
// object_to_world.transform_surface_interaction (src/core/transform.rs:815-860), written from the reference's text over the helpers of
// tests/sphere_restated.cpp (EFloat, quadratic, the transforms with their error terms), and a walk of an rspt_bvh_node array in
// BVHAccel::intersect / intersect_p's order (bvh.rs:401-514) over triangles, spheres, disks and cylinders.
// f32 throughout with the host libm (atan2f), the discriminant in f64; build with -ffp-contract=off.
// Nothing compiled from the reference holds this file: tests/test_quadric_host.py holds it to closed-form answers instead.
#ifndef QUADRIC_RESTATED_HAVE_SPHERE   // (tests/quadric_render_restated.cpp has included it through tests/sphere_render_restated.cpp)
#include "sphere_restated.cpp"
#endif

namespace {

// Ray::position (geometry.rs): o + d * t
V position(V o, V d, float t) { return add(o, mul(d, t)); }
// Vector3f / f32 (geometry.rs:1271-1279): a multiplication by the reciprocal
V vdiv(V a, float b) { const float inv = 1.0f / b; return V{a.x * inv, a.y * inv, a.z * inv}; }

// transform_ray_with_error (transform.rs:793-814): t_max is kept
void object_ray(const float* w2o, V wo, V wd, V* o_out, V* d_out, V* o_err, V* d_err) {
    V o = point_with_error(w2o, wo, o_err);
    const V d = vector_with_error(w2o, wd, d_err);
    const float ls = vdot(d, d);
    if (ls > 0.0f) {
        const float dt = vdot(vabs(d), *o_err) / ls;
        o = add(o, mul(d, dt));
    }
    *o_out = o; *d_out = d;
}

// SurfaceInteraction::new with shape None (interaction.rs:259-280: n = normalize(cross(dpdu, dpdv)), no flip, the shading frame a copy) followed by
// object_to_world.transform_surface_interaction (transform.rs:815-860)
void to_world(const float* m, const float* mi, float t, V ph, V perr, float u, float v, V dpdu, V dpdv, V dndu, V dndv, Hit* h) {
    const V n = vnormalize(vcross(dpdu, dpdv));
    const float g3 = gamma(3);
    const float xp = m[0] * ph.x + m[1] * ph.y + m[2] * ph.z + m[3];
    const float yp = m[4] * ph.x + m[5] * ph.y + m[6] * ph.z + m[7];
    const float zp = m[8] * ph.x + m[9] * ph.y + m[10] * ph.z + m[11];
    const float wp = m[12] * ph.x + m[13] * ph.y + m[14] * ph.z + m[15];
    float ae[3];
    for (int r = 0; r < 3; r++) {   // transform_point_with_abs_error (transform.rs:709-769)
        const float* row = m + 4 * r;
        ae[r] = (g3 + 1.0f) * (std::fabs(row[0]) * perr.x + std::fabs(row[1]) * perr.y + std::fabs(row[2]) * perr.z) +
                g3 * (std::fabs(row[0] * ph.x) + std::fabs(row[1] * ph.y) + std::fabs(row[2] * ph.z) + std::fabs(row[3]));
    }
    h->t = t;
    h->p_error = V{ae[0], ae[1], ae[2]};
    if (wp == 1.0f) h->p = V{xp, yp, zp};
    else { const float inv = 1.0f / wp; h->p = V{inv * xp, inv * yp, inv * zp}; }
    h->n = vnormalize(xnrm(mi, n));
    h->u = u; h->v = v;
    h->dpdu = xvec(m, dpdu); h->dpdv = xvec(m, dpdv); h->dndu = xnrm(mi, dndu); h->dndv = xnrm(mi, dndv);
    V sn = vnormalize(xnrm(mi, n));
    if (vdot(sn, h->n) < 0.0f) sn = V{-sn.x, -sn.y, -sn.z};   // nrm_faceforward_nrm
    h->sn = sn; h->sdpdu = h->dpdu; h->sdpdv = h->dpdv; h->sdndu = h->dndu; h->sdndv = h->dndv;
}

// Disk::intersect (full = true, disk.rs:92-162) / intersect_p (full = false, :163-197)
bool disk_intersect(const rspt_disk& s, V wo, V wd, float t_max, bool full, Hit* h) {
    V o, d, o_err, d_err;
    object_ray(s.world_to_object, wo, wd, &o, &d, &o_err, &d_err);
    if (d.z == 0.0f) return false;                                   // :104
    const float t_shape_hit = (s.height - o.z) / d.z;                // :107
    if (t_shape_hit <= 0.0f || t_shape_hit >= t_max) return false;   // :108
    V p_hit = position(o, d, t_shape_hit);
    const float dist2 = p_hit.x * p_hit.x + p_hit.y * p_hit.y;
    if (dist2 > s.radius * s.radius || dist2 < s.inner_radius * s.inner_radius) return false;   // :114
    float phi = std::atan2(p_hit.y, p_hit.x);
    if (phi < 0.0f) phi += 2.0f * (float)M_PI;
    if (phi > s.phi_max) return false;
    h->t = t_shape_hit;
    if (!full) return true;
    const float u = phi / s.phi_max;
    const float r_hit = std::sqrt(dist2);
    const float one_minus_v = (r_hit - s.inner_radius) / (s.radius - s.inner_radius);
    const float v = 1.0f - one_minus_v;
    const V dpdu{-s.phi_max * p_hit.y, s.phi_max * p_hit.x, 0.0f};
    const V dpdv = vdiv(mul(V{p_hit.x, p_hit.y, 0.0f}, s.inner_radius - s.radius), r_hit);   // :135-140
    const V zero{0.0f, 0.0f, 0.0f};
    p_hit.z = s.height;   // :144, after dist2 and phi
    to_world(s.object_to_world, s.world_to_object, t_shape_hit, p_hit, zero /* p_error, :146 */, u, v, dpdu, dpdv, zero, zero, h);
    return true;
}

// Cylinder::intersect (full = true, cylinder.rs:95-245) / intersect_p (full = false, :246-321)
bool cylinder_intersect(const rspt_cylinder& s, V wo, V wd, float t_max, bool full, Hit* h) {
    V o, d, o_err, d_err;
    object_ray(s.world_to_object, wo, wd, &o, &d, &o_err, &d_err);
    const EFloat ox = ef(o.x, o_err.x), oy = ef(o.y, o_err.y);
    const EFloat dx = ef(d.x, d_err.x), dy = ef(d.y, d_err.y);
    const EFloat a = dx * dx + dy * dy;
    const EFloat b = (dx * ox + dy * oy) * 2.0f;
    const EFloat c = ox * ox + oy * oy - ef(s.radius, 0.0f) * ef(s.radius, 0.0f);
    EFloat t0, t1;
    if (!quadratic(a, b, c, &t0, &t1)) return false;
    if (t0.high > t_max || t1.low <= 0.0f) return false;   // :125
    EFloat ts = t0;
    if (ts.low <= 0.0f) {
        ts = t1;
        if (ts.high > t_max) return false;
    }
    auto hit_point = [&](float t, V* p, float* phi) {   // :136-144
        V q = position(o, d, t);
        const float hit_rad = std::sqrt(q.x * q.x + q.y * q.y);
        q.x *= s.radius / hit_rad;
        q.y *= s.radius / hit_rad;
        float f = std::atan2(q.y, q.x);
        if (f < 0.0f) f += 2.0f * (float)M_PI;
        *p = q; *phi = f;
    };
    auto clipped = [&](V p, float phi) { return p.z < s.z_min || p.z > s.z_max || phi > s.phi_max; };
    V ph;
    float phi;
    hit_point(ts.v, &ph, &phi);
    if (clipped(ph, phi)) {   // :146-168
        if (ts.v == t1.v) return false;
        ts = t1;
        if (t1.high > t_max) return false;
        hit_point(ts.v, &ph, &phi);
        if (clipped(ph, phi)) return false;
    }
    h->t = ts.v;
    if (!full) return true;
    const float u = phi / s.phi_max;
    const float v = (ph.z - s.z_min) / (s.z_max - s.z_min);
    const V dpdu{-s.phi_max * ph.y, s.phi_max * ph.x, 0.0f};
    const V dpdv{0.0f, 0.0f, s.z_max - s.z_min};
    const V d2duu = mul(mul(V{ph.x, ph.y, 0.0f}, -s.phi_max), s.phi_max);
    const V d2duv{0.0f, 0.0f, 0.0f}, d2dvv{0.0f, 0.0f, 0.0f};
    const float E = vdot(dpdu, dpdu), F = vdot(dpdu, dpdv), G = vdot(dpdv, dpdv);
    const V nc = vnormalize(vcross(dpdu, dpdv));
    const float e = vdot(nc, d2duu), f = vdot(nc, d2duv), g = vdot(nc, d2dvv);
    const float inv_egf2 = 1.0f / (E * G - F * F);
    const V dndu = add(mul(mul(dpdu, f * F - e * G), inv_egf2), mul(mul(dpdv, e * F - f * E), inv_egf2));
    const V dndv = add(mul(mul(dpdu, g * F - f * G), inv_egf2), mul(mul(dpdv, f * F - g * E), inv_egf2));
    const V perr = mul(vabs(V{ph.x, ph.y, 0.0f}), gamma(3));   // :223-229
    to_world(s.object_to_world, s.world_to_object, ts.v, ph, perr, u, v, dpdu, dpdv, dndu, dndv, h);
    return true;
}

// a Hit in the hook's output layout
void emit(const Hit& h, float* r) {
    const V v[13] = {h.p, h.p_error, h.n, V{h.u, h.v, 0.0f}, h.dpdu, h.dpdv, h.dndu, h.dndv, h.sn, h.sdpdu, h.sdpdv, h.sdndu, h.sdndv};
    r[0] = 1.0f; r[1] = h.t;
    int k = 2;
    for (int j = 0; j < 13; j++) { r[k++] = v[j].x; r[k++] = v[j].y; if (j != 3) r[k++] = v[j].z; }
}

}  // namespace

extern "C" {
// the layout of rspt_quadric_intersect (include/rspt.h): 64 floats in, 64 out per element; shape = RSPT_MESH_SPHERE | _DISK | _CYLINDER
int quad_hook(uint32_t shape, const float* x, uint64_t n, float* out) {
    if (shape != RSPT_MESH_SPHERE && shape != RSPT_MESH_DISK && shape != RSPT_MESH_CYLINDER) return -1;
    const int words = shape == RSPT_MESH_SPHERE ? 42 : 40;
    for (uint64_t i = 0; i < n; i++) {
        const float* q = x + 64 * i + words;
        float* r = out + 64 * i;
        for (int k = 0; k < 64; k++) r[k] = 0.0f;
        const V o{q[0], q[1], q[2]}, d{q[3], q[4], q[5]};
        Hit h, hp;
        bool full, any;
        if (shape == RSPT_MESH_DISK) {
            rspt_disk s;
            std::memcpy(&s, x + 64 * i, sizeof s);
            full = disk_intersect(s, o, d, q[6], true, &h); any = disk_intersect(s, o, d, q[6], false, &hp);
        } else if (shape == RSPT_MESH_CYLINDER) {
            rspt_cylinder s;
            std::memcpy(&s, x + 64 * i, sizeof s);
            full = cylinder_intersect(s, o, d, q[6], true, &h); any = cylinder_intersect(s, o, d, q[6], false, &hp);
        } else {
            rspt_sphere s;
            std::memcpy(&s, x + 64 * i, sizeof s);
            full = sphere_intersect(s, o, d, q[6], true, &h); any = sphere_intersect(s, o, d, q[6], false, &hp);
        }
        if (full) emit(h, r);
        r[43] = any ? 1.0f : 0.0f;
    }
    return 0;
}

// BVHAccel::intersect (any = 0) / intersect_p (any = 1) over triangles (the oracle's watertight test), spheres, disks and cylinders.  Meshes with an
// alpha mask are given a constant-0 mask by the tests: no candidate on them is ever a hit (triangle.rs:313-330, :593-655).
void quad_walk(const rspt_scene_desc* desc, const rspt_ray* rays, uint64_t n, int any, rspt_hit* out) {
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
                            const V o{ray.o.x, ray.o.y, ray.o.z}, d{ray.d.x, ray.d.y, ray.d.z};
                            bool h;
                            Hit sh;
                            if (pr.mesh == RSPT_MESH_SPHERE) { h = sphere_intersect(desc->spheres[pr.v[0]], o, d, ray.t_max, false, &sh); t = sh.t; }
                            else if (pr.mesh == RSPT_MESH_DISK) { h = disk_intersect(desc->disks[pr.v[0]], o, d, ray.t_max, false, &sh); t = sh.t; }
                            else if (pr.mesh == RSPT_MESH_CYLINDER) { h = cylinder_intersect(desc->cylinders[pr.v[0]], o, d, ray.t_max, false, &sh); t = sh.t; }
                            else h = sc.tri_hit_test(pr, ray, &t, b) && !(desc->meshes[pr.mesh].alpha_tex || desc->meshes[pr.mesh].shadow_alpha_tex);
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
