// RealisticCamera (src/cameras/realistic.rs) restated operation by operation in f32 (the quadratic's discriminant in f64), uncontracted: the lens-system
// tracer of the raygen kernel (ABI 26) and, on the host, of rspt_realistic_camera_setup.  One text serves both: the functions of the first part are
// __host__ __device__ and read the interface table through whatever pointer they are given.
//   lens_flip_ray               camera_to_lens / lens_to_camera = Transform::scale(1, 1, -1).transform_ray (transform.rs:538-595 with
//                               transform_point_with_error :662-708): the origin moves along d by the error-bound term and t_max shrinks, both ways
//   lens_quadratic              pbrt.rs:248-268
//   lens_intersect_spherical    intersect_spherical_element (:328-365)
//   lens_trace_from_film        trace_lenses_from_film (:266-327)
//   lens_trace_from_scene       trace_lenses_from_scene (:366-421; the setup's thick-lens approximation only)
//   lens_sample_exit_pupil      sample_exit_pupil (:656-688)
//   lens_camera_ray             generate_ray (:198-251) up to the camera-space ray and its weight
//   lens_ray_differential       generate_ray_differential (:693-735): device only, over camera_to_world_at / the transform_ray tail of dev_scene.h
#pragma once
#include "dev_scene.h"

namespace rspt {

#define LHD __host__ __device__ inline
struct lv3 { float x, y, z; };
LHD lv3 lv_add(lv3 a, lv3 b) { return lv3{a.x + b.x, a.y + b.y, a.z + b.z}; }
LHD lv3 lv_sub(lv3 a, lv3 b) { return lv3{a.x - b.x, a.y - b.y, a.z - b.z}; }
LHD lv3 lv_neg(lv3 a) { return lv3{-a.x, -a.y, -a.z}; }
LHD lv3 lv_mul(lv3 a, float s) { return lv3{a.x * s, a.y * s, a.z * s}; }
LHD lv3 lv_div(lv3 a, float s) { const float inv = 1.0f / s; return lv3{a.x * inv, a.y * inv, a.z * inv}; }   // geometry.rs:1261-1297: times the reciprocal
LHD float lv_dot(lv3 a, lv3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
LHD lv3 lv_normalize(lv3 a) { return lv_div(a, sqrtf(lv_dot(a, a))); }
LHD float lens_lerp(float t, float a, float b) { return a * (1.0f - t) + b * t; }   // pbrt.rs:231-241

struct LensRay { lv3 o, d; float t_max; };
// what the tracer reads of a RealisticCamera: element_interfaces, exit_pupil_bounds (p_min.x, p_min.y, p_max.x, p_max.y each), Film::diagonal,
// Film::full_resolution, simple_weighting and the shutter
struct LensSystem {
    const rspt_lens_element* elements;
    const float* bounds;
    uint32_t n_elements, n_bounds;
    float film_diagonal, res_x, res_y, shutter_open, shutter_close;
    uint32_t simple_weighting;
};

LHD LensRay lens_flip_ray(const LensRay& r) {
    const float m[16] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    const float x = r.o.x, y = r.o.y, z = r.o.z;
    const float xp = m[0] * x + m[1] * y + m[2] * z + m[3];
    const float yp = m[4] * x + m[5] * y + m[6] * z + m[7];
    const float zp = m[8] * x + m[9] * y + m[10] * z + m[11];
    const float wp = m[12] * x + m[13] * y + m[14] * z + m[15];
    const float xs = fabsf(m[0] * x) + fabsf(m[1] * y) + fabsf(m[2] * z) + fabsf(m[3]);
    const float ys = fabsf(m[4] * x) + fabsf(m[5] * y) + fabsf(m[6] * z) + fabsf(m[7]);
    const float zs = fabsf(m[8] * x) + fabsf(m[9] * y) + fabsf(m[10] * z) + fabsf(m[11]);
    const float g3 = (3.0f * 5.9604645e-8f) / (1.0f - 3.0f * 5.9604645e-8f);   // gamma(3), pbrt.rs:94-96
    const lv3 o_err{xs * g3, ys * g3, zs * g3};
    lv3 o{xp, yp, zp};
    if (wp != 1.0f) { const float inv = 1.0f / wp; o = lv3{inv * xp, inv * yp, inv * zp}; }
    const lv3 d{m[0] * r.d.x + m[1] * r.d.y + m[2] * r.d.z, m[4] * r.d.x + m[5] * r.d.y + m[6] * r.d.z, m[8] * r.d.x + m[9] * r.d.y + m[10] * r.d.z};
    const float ls = lv_dot(d, d);
    float t_max = r.t_max;
    if (ls > 0.0f) {
        const float dt = lv_dot(lv3{fabsf(d.x), fabsf(d.y), fabsf(d.z)}, o_err) / ls;
        o = lv_add(o, lv_mul(d, dt));
        t_max -= dt;
    }
    return LensRay{o, d, t_max};
}
// the discriminant, its root and q in f64; t0 = (q as f32) / a and t1 = c / (q as f32) in f32; then the swap
LHD bool lens_quadratic(float a, float b, float c, float* t0, float* t1) {
    const double discrim = (double)b * (double)b - 4.0 * (double)a * (double)c;
    if (discrim < 0.0) return false;
    const double root = sqrt(discrim);
    const double q = b < 0.0f ? -0.5 * ((double)b - root) : -0.5 * ((double)b + root);
    *t0 = (float)q / a;
    *t1 = c / (float)q;
    if (*t0 > *t1) { const float s = *t0; *t0 = *t1; *t1 = s; }
    return true;
}
LHD bool lens_intersect_spherical(float radius, float z_center, const LensRay& ray, float* t, lv3* n) {
    const lv3 o = lv_sub(ray.o, lv3{0.0f, 0.0f, z_center});
    const float a = ray.d.x * ray.d.x + ray.d.y * ray.d.y + ray.d.z * ray.d.z;
    const float b = 2.0f * (ray.d.x * o.x + ray.d.y * o.y + ray.d.z * o.z);
    const float c = o.x * o.x + o.y * o.y + o.z * o.z - radius * radius;
    float t0 = 0.0f, t1 = 0.0f;
    if (!lens_quadratic(a, b, c, &t0, &t1)) return false;
    const bool use_closer_t = (ray.d.z > 0.0f) ^ (radius < 0.0f);
    *t = use_closer_t ? fminf(t0, t1) : fmaxf(t0, t1);
    if (*t < 0.0f) return false;
    const lv3 nn = lv_normalize(lv_add(o, lv_mul(ray.d, *t)));
    *n = lv_dot(nn, lv_neg(ray.d)) < 0.0f ? lv_neg(nn) : nn;   // nrm_faceforward_vec3(n.normalize(), -ray.d)
    return true;
}
LHD bool lens_refract(lv3 wi, lv3 n, float eta, lv3* wt) {   // reflection.rs:1897-1909
    const float ci = lv_dot(n, wi);
    const float s2i = fmaxf(0.0f, 1.0f - ci * ci);
    const float s2t = eta * eta * s2i;
    if (s2t >= 1.0f) return false;
    const float ct = sqrtf(1.0f - s2t);
    *wt = lv_add(lv_mul(lv_neg(wi), eta), lv_mul(n, eta * ci - ct));
    return true;
}
// t_neg (may be null): counts the interfaces at which the reference's assert!(t >= 0) would have fired; the trace goes on with that t
LHD bool lens_trace_from_film(const rspt_lens_element* el, uint32_t n_el, const LensRay& r_camera, LensRay* r_out, uint32_t* t_neg) {
    float element_z = 0.0f;
    LensRay r = lens_flip_ray(r_camera);
    for (uint32_t idx = 0; idx < n_el; idx++) {
        const uint32_t i = n_el - 1u - idx;
        const rspt_lens_element e = el[i];
        element_z -= e.thickness;
        float t = 0.0f;
        lv3 n{0.0f, 0.0f, 0.0f};
        const bool is_stop = e.curvature_radius == 0.0f;
        if (is_stop) {
            if (r.d.z >= 0.0f) return false;   // before the division: a ray refracted back towards the film
            t = (element_z - r.o.z) / r.d.z;
        } else if (!lens_intersect_spherical(e.curvature_radius, element_z + e.curvature_radius, r, &t, &n))
            return false;
        if (t_neg && !(t >= 0.0f)) *t_neg += 1u;
        const lv3 p_hit = lv_add(r.o, lv_mul(r.d, t));
        const float r2 = p_hit.x * p_hit.x + p_hit.y * p_hit.y;
        if (r2 > e.aperture_radius * e.aperture_radius) return false;
        r.o = p_hit;
        if (!is_stop) {
            const float eta_i = e.eta;
            const float eta_t = (i > 0u && el[i - 1u].eta != 0.0f) ? el[i - 1u].eta : 1.0f;
            lv3 w;
            if (!lens_refract(lv_normalize(lv_neg(r.d)), n, eta_i / eta_t, &w)) return false;
            r.d = w;
        }
    }
    if (r_out) *r_out = lens_flip_ray(r);
    return true;
}
LHD float lens_front_z(const rspt_lens_element* el, uint32_t n_el) {
    float z = 0.0f;
    for (uint32_t i = 0; i < n_el; i++) z += el[i].thickness;
    return z;
}
LHD bool lens_trace_from_scene(const rspt_lens_element* el, uint32_t n_el, const LensRay& r_camera, LensRay* r_out, uint32_t* t_neg) {
    float element_z = -lens_front_z(el, n_el);
    LensRay r = lens_flip_ray(r_camera);
    for (uint32_t i = 0; i < n_el; i++) {
        const rspt_lens_element e = el[i];
        float t = 0.0f;
        lv3 n{0.0f, 0.0f, 0.0f};
        const bool is_stop = e.curvature_radius == 0.0f;
        if (is_stop) t = (element_z - r.o.z) / r.d.z;
        else if (!lens_intersect_spherical(e.curvature_radius, element_z + e.curvature_radius, r, &t, &n)) return false;
        if (t_neg && !(t >= 0.0f)) *t_neg += 1u;
        const lv3 p_hit = lv_add(r.o, lv_mul(r.d, t));
        const float r2 = p_hit.x * p_hit.x + p_hit.y * p_hit.y;
        if (r2 > e.aperture_radius * e.aperture_radius) return false;
        r.o = p_hit;
        if (!is_stop) {
            const float eta_i = (i == 0u || el[i - 1u].eta == 0.0f) ? 1.0f : el[i - 1u].eta;
            const float eta_t = e.eta != 0.0f ? e.eta : 1.0f;
            lv3 w;
            if (!lens_refract(lv_normalize(lv_neg(r.d)), n, eta_i / eta_t, &w)) return false;
            r.d = w;
        }
        element_z += e.thickness;
    }
    if (r_out) *r_out = lens_flip_ray(r);
    return true;
}
LHD lv3 lens_sample_exit_pupil(const LensSystem& L, float fx, float fy, float lx, float ly, float* area) {
    const float r_film = sqrtf(fx * fx + fy * fy);
    const float fi = floorf(r_film / (L.film_diagonal / 2.0f) * (float)L.n_bounds);
    uint32_t r_index = 0u;   // `as usize` saturates, NaN -> 0; then min(len - 1, .)
    if (fi >= (float)(L.n_bounds - 1u)) r_index = L.n_bounds - 1u;
    else if (fi > 0.0f) r_index = (uint32_t)fi;
    const float* b = L.bounds + 4u * r_index;
    const float x0 = b[0], y0 = b[1], x1 = b[2], y1 = b[3];
    *area = (x1 - x0) * (y1 - y0);
    const float px = lens_lerp(lx, x0, x1), py = lens_lerp(ly, y0, y1);
    const float sin_theta = r_film != 0.0f ? fy / r_film : 0.0f;
    const float cos_theta = r_film != 0.0f ? fx / r_film : 1.0f;
    return lv3{cos_theta * px - sin_theta * py, sin_theta * px + cos_theta * py, L.elements[L.n_elements - 1u].thickness};
}
// generate_ray (:198-251) without its camera_to_world step: the camera-space ray behind the lens and the ray weight (0: vignetted, *out untouched)
LHD float lens_camera_ray(const LensSystem& L, float film_x, float film_y, float lens_x, float lens_y, LensRay* out, uint32_t* t_neg) {
    const float sx = film_x / L.res_x, sy = film_y / L.res_y;
    const float aspect = L.res_y / L.res_x;                                                        // Film::get_physical_extent (film.rs:293-307)
    const float ex = sqrtf(L.film_diagonal * L.film_diagonal / (1.0f + aspect * aspect)), ey = aspect * ex;
    const float p2x = lens_lerp(sx, -ex / 2.0f, ex / 2.0f), p2y = lens_lerp(sy, -ey / 2.0f, ey / 2.0f);
    const lv3 p_film{-p2x, p2y, 0.0f};
    float area = 0.0f;
    const lv3 p_rear = lens_sample_exit_pupil(L, p_film.x, p_film.y, lens_x, lens_y, &area);
    const LensRay r_film{p_film, lv_sub(p_rear, p_film), __builtin_huge_valf()};
    if (!lens_trace_from_film(L.elements, L.n_elements, r_film, out, t_neg)) return 0.0f;
    const float cos_theta = lv_normalize(r_film.d).z;
    const float cos2 = cos_theta * cos_theta, cos4 = cos2 * cos2;
    if (L.simple_weighting) {
        const float* b0 = L.bounds;
        return cos4 * area / ((b0[2] - b0[0]) * (b0[3] - b0[1]));
    }
    const float rear_z = L.elements[L.n_elements - 1u].thickness;
    return (L.shutter_close - L.shutter_open) * (cos4 * area) / (rear_z * rear_z);
}
LHD float lens_radical_inverse(int base_index, uint64_t a) {   // lowdiscrepancy.rs:1082-1135, bases 2 and 3
    if (base_index == 0) {
        uint64_t v = a;
        v = (v << 32) | (v >> 32);
        v = ((v & 0x0000ffff0000ffffull) << 16) | ((v & 0xffff0000ffff0000ull) >> 16);
        v = ((v & 0x00ff00ff00ff00ffull) << 8) | ((v & 0xff00ff00ff00ff00ull) >> 8);
        v = ((v & 0x0f0f0f0f0f0f0f0full) << 4) | ((v & 0xf0f0f0f0f0f0f0f0ull) >> 4);
        v = ((v & 0x3333333333333333ull) << 2) | ((v & 0xccccccccccccccccull) >> 2);
        v = ((v & 0x5555555555555555ull) << 1) | ((v & 0xaaaaaaaaaaaaaaaaull) >> 1);
        return (float)v * 0x1.0p-64f;
    }
    const uint64_t base = 3;
    const float inv_base = 1.0f / (float)base;
    uint64_t reversed = 0;
    float inv_base_n = 1.0f;
    while (a != 0) {
        const uint64_t next = a / base, digit = a - next * base;
        reversed = reversed * base + digit;
        inv_base_n *= inv_base;
        a = next;
    }
    return fminf((float)reversed * inv_base_n, 0x1.fffffep-1f);
}
// bound_exit_pupil (:573-652): out = p_min.x, p_min.y, p_max.x, p_max.y
LHD void lens_bound_exit_pupil(const rspt_lens_element* el, uint32_t n_el, float x0, float x1, float out[4], uint32_t* t_neg) {
    float bx0 = 0.0f, by0 = 0.0f, bx1 = 0.0f, by1 = 0.0f;   // Bounds2f::default(): the point (0, 0)
    const int32_t n_samples = 1024 * 1024;
    int32_t n_exiting = 0;
    const float rear_radius = el[n_el - 1u].aperture_radius, rear_z = el[n_el - 1u].thickness;
    const float lo = -1.5f * rear_radius, hi = 1.5f * rear_radius;
    for (int32_t i = 0; i < n_samples; i++) {
        const lv3 p_film{lens_lerp(((float)i + 0.5f) / (float)n_samples, x0, x1), 0.0f, 0.0f};
        const float u0 = lens_radical_inverse(0, (uint64_t)i), u1 = lens_radical_inverse(1, (uint64_t)i);
        const lv3 p_rear{lens_lerp(u0, lo, hi), lens_lerp(u1, lo, hi), rear_z};
        const bool inside = p_rear.x >= bx0 && p_rear.x <= bx1 && p_rear.y >= by0 && p_rear.y <= by1;
        if (inside || lens_trace_from_film(el, n_el, LensRay{p_film, lv_sub(p_rear, p_film), __builtin_huge_valf()}, nullptr, t_neg)) {
            bx0 = fminf(bx0, p_rear.x); by0 = fminf(by0, p_rear.y);
            bx1 = fmaxf(bx1, p_rear.x); by1 = fmaxf(by1, p_rear.y);
            n_exiting++;
        }
    }
    if (n_exiting == 0) { out[0] = lo; out[1] = lo; out[2] = hi; out[3] = hi; return; }
    const float dx = hi - lo, dy = hi - lo;
    const float delta = 2.0f * sqrtf(dx * dx + dy * dy) / sqrtf((float)n_samples);
    out[0] = bx0 - delta; out[1] = by0 - delta; out[2] = bx1 + delta; out[3] = by1 + delta;
}

// ---- device: the world-space ray with its differentials ----
struct LensRayOut { f3 o, d; float t_max, time; f3 rx_o, rx_d, ry_o, ry_d; };   // what generate_ray_differential leaves in `ray` (differentials: zeros unless the weight is > 0)
struct LensTraced { LensRay r; float w; };   // r.t_max = 0: the trace failed and the ray is still Ray::default()
// The one call site of the lens trace: not inlined, so that the five traces of a sample are five passes of one loop over one body (inlined, the
// quadratic's f64 and the refraction would be laid out five times).  Everything travels by value: a pointer to the kernel's argument would put it into scratch.
__device__ __noinline__ LensTraced lens_camera_ray_call(LensSystem L, float film_x, float film_y, float lens_x, float lens_y) {
    LensTraced t{LensRay{lv3{0.0f, 0.0f, 0.0f}, lv3{0.0f, 0.0f, 0.0f}, 0.0f}, 0.0f};
    t.w = lens_camera_ray(L, film_x, film_y, lens_x, lens_y, &t.r, nullptr);
    return t;
}
// The shifted rays are traced for every sample (the weight depends on them), the second sign of a shift only when the first gave weight 0; a shift may
// land in another exit-pupil band and find a quite different lens point: the reference's behaviour.
RDEV float lens_ray_differential(const RenderDev& rd, const LensSystem& L, float film_x, float film_y, float time_s, float lens_x, float lens_y, LensRayOut* ray) {
    const f3 zero{0.0f, 0.0f, 0.0f};
    *ray = LensRayOut{zero, zero, 0.0f, 0.0f, zero, zero, zero, zero};   // Ray::default()
    float c2w[16];
    camera_to_world_at(rd, time_s, c2w);   // AnimatedTransform::transform_ray at the ray's time (transform.rs:2114-2124)
    const float time = rd.shutter_open * (1.0f - time_s) + rd.shutter_close * time_s;
    float wt = 0.0f, wtx = 0.0f, wty = 0.0f;
#pragma unroll 1
    for (int k = 0; k < 5; k++) {   // 0: the ray itself; 1, 2: p_film.x + 0.05, - 0.05; 3, 4: p_film.y + 0.05, - 0.05
        if ((k == 2 && wtx != 0.0f) || (k == 4 && wty != 0.0f)) continue;
        if (k == 3 && wtx == 0.0f) break;
        const float eps = (k & 1) ? 0.05f : -0.05f;
        const float fx = (k == 1 || k == 2) ? film_x + eps : film_x, fy = k >= 3 ? film_y + eps : film_y;
        const LensTraced tr = lens_camera_ray_call(L, fx, fy, lens_x, lens_y);
        f3 ow = zero, dw = zero;
        float t_max = 0.0f;
        const bool traced = tr.r.t_max != 0.0f;
        if (traced) {   // *ray = camera_to_world.transform_ray(ray); ray.d = ray.d.normalize() (:234-235); else the ray stays Ray::default()
            f3 o_err;
            ow = xf_point_err(c2w, f3{tr.r.o.x, tr.r.o.y, tr.r.o.z}, &o_err);
            dw = xf_vector(c2w, f3{tr.r.d.x, tr.r.d.y, tr.r.d.z});
            const float ls = len2(dw);
            t_max = tr.r.t_max;
            if (ls > 0.0f) {
                const float dt = dot(vabs(dw), o_err) / ls;
                ow = ow + dw * dt;
                t_max -= dt;
            }
            dw = normalize(dw);
        }
        if (k == 0) {
            wt = tr.w;
            if (traced) { ray->o = ow; ray->d = dw; ray->t_max = t_max; ray->time = time; }
            if (wt == 0.0f) break;
            continue;
        }
        const f3 so = ray->o + vdiv(ow - ray->o, eps), sd = ray->d + vdiv(dw - ray->d, eps);
        if (k <= 2) { wtx = tr.w; ray->rx_o = so; ray->rx_d = sd; }
        else { wty = tr.w; ray->ry_o = so; ray->ry_d = sd; }
    }
    if (wt == 0.0f || wtx == 0.0f || wty == 0.0f) { ray->rx_o = ray->rx_d = ray->ry_o = ray->ry_d = zero; return 0.0f; }
    return wt;
}

}  // namespace rspt
