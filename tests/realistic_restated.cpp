// The CPU yardstick of the realistic camera (ABI 26).  The oracle knows the perspective camera only and tests/camera_restated.cpp fixes ray_weight = 1, so this
// file holds
//   (a) RealisticCamera (src/cameras/realistic.rs) written from the reference's text over the oracle's leaf functions: generate_ray (:198-251),
//       trace_lenses_from_film (:266-327), intersect_spherical_element (:328-365), trace_lenses_from_scene (:366-421), compute_cardinal_points /
//       compute_thick_lens_approximation / focus_thick_lens (:431-499), bound_exit_pupil (:573-652), sample_exit_pupil (:656-688),
//       generate_ray_differential (:693-735), quadratic (pbrt.rs:248-268), and the state RealisticCamera::new builds (:50-144; focus_binary_search, :92,
//       is left out: its result is discarded there);
//   (b) real_render: orc::render's tile loop (SamplerIntegrator::render, integrator.rs:70-220) once more, with the camera chosen by rd->camera_kind
//       (0: the oracle's camera_ray), a real ray_weight into FilmTile::add_sample, and `if ray_weight > 0 { li }` (:149);
//   (c) an extern "C" surface.
// tests/test_realistic_host.py holds (b) with camera_kind = 0 to orc::render bit for bit, the library's setup to (a)'s, and (a) to known answers;
// tests/test_gpu_realistic.py holds rspt_camera_rays and rspt_render to this file.
// Built by the tests: g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared -I oracle -I include -I tests.
// -DCAM_LI_SPHERES (with tests/sphere_render_restated.cpp linked in): real_render installs that file's li restatements, as tests/camera_restated.cpp does.
#include "orc_render.hpp"

namespace orc {
#ifdef CAM_LI_SPHERES
namespace sphr { Spec path_li(RenderCtx& cx, const Ray& r, Sampler& sampler, Counters* c); Spec ao_li(RenderCtx& cx, const Ray& ray, Sampler& sampler, Counters* c); }
#endif
namespace real {

static std::atomic<uint64_t> g_t_neg{0};   // how often assert!(t >= 0.0) (:297, :386) would have fired

struct Bounds2 { P2 p_min{0.0f, 0.0f}, p_max{0.0f, 0.0f};   // #[derive(Default)]: the point (0, 0)
    Float area() const { return (p_max.x - p_min.x) * (p_max.y - p_min.y); }
    P2 lerp2(P2 t) const { return P2{lerp(t.x, p_min.x, p_max.x), lerp(t.y, p_min.y, p_max.y)}; }
    bool inside(P2 p) const { return p.x >= p_min.x && p.x <= p_max.x && p.y >= p_min.y && p.y <= p_max.y; }
};
struct Camera {
    std::vector<rspt_lens_element> el;       // element_interfaces
    std::vector<Bounds2> pupil;              // exit_pupil_bounds
    Float diagonal = 0.0f;                   // film.diagonal (metres)
    int32_t res[2] = {1, 1};                 // film.full_resolution
    Float shutter_open = 0.0f, shutter_close = 1.0f;
    bool simple_weighting = true;
    Float lens_rear_z() const { return el.back().thickness; }
    Float lens_front_z() const { Float z = 0.0f; for (const auto& e : el) z += e.thickness; return z; }
    Float rear_element_radius() const { return el.back().aperture_radius; }
};
static const Float SCALE_Z[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1};   // Transform::scale(1, 1, -1).m

static inline bool quadratic(Float a, Float b, Float c, Float* t0, Float* t1) {   // pbrt.rs:248-268
    const double discrim = (double)b * (double)b - 4.0 * (double)a * (double)c;
    if (discrim < 0.0) return false;
    const double root_discrim = std::sqrt(discrim);
    const double q = b < 0.0f ? -0.5 * ((double)b - root_discrim) : -0.5 * ((double)b + root_discrim);
    *t0 = (Float)q / a;
    *t1 = c / (Float)q;
    if (*t0 > *t1) std::swap(*t0, *t1);
    return true;
}
static inline bool intersect_spherical_element(Float radius, Float z_center, const Ray& ray, Float* t, V3* n) {   // :328-365
    const V3 o = ray.o - V3{0.0f, 0.0f, z_center};
    const Float a = ray.d.x * ray.d.x + ray.d.y * ray.d.y + ray.d.z * ray.d.z;
    const Float b = 2.0f * (ray.d.x * o.x + ray.d.y * o.y + ray.d.z * o.z);
    const Float c = o.x * o.x + o.y * o.y + o.z * o.z - radius * radius;
    Float t0 = 0.0f, t1 = 0.0f;
    if (!quadratic(a, b, c, &t0, &t1)) return false;
    const bool use_closer_t = (ray.d.z > 0.0f) ^ (radius < 0.0f);
    *t = use_closer_t ? std::fmin(t0, t1) : std::fmax(t0, t1);
    if (*t < 0.0f) return false;
    *n = o + ray.d * *t;
    *n = faceforward(normalize(*n), -ray.d);
    return true;
}
static inline bool trace_lenses_from_film(const Camera& cam, const Ray& r_camera, Ray* r_out) {   // :266-327
    Float element_z = 0.0f;
    Ray r_lens = transform_ray(SCALE_Z, r_camera);
    const size_t ei_len = cam.el.size();
    for (size_t idx = 0; idx < ei_len; idx++) {
        const size_t i = ei_len - 1 - idx;
        const rspt_lens_element element = cam.el[i];
        element_z -= element.thickness;
        Float t = 0.0f;
        V3 n{0.0f, 0.0f, 0.0f};
        const bool is_stop = element.curvature_radius == 0.0f;
        if (is_stop) {
            if (r_lens.d.z >= 0.0f) return false;
            t = (element_z - r_lens.o.z) / r_lens.d.z;
        } else {
            const Float radius = element.curvature_radius;
            const Float z_center = element_z + element.curvature_radius;
            if (!intersect_spherical_element(radius, z_center, r_lens, &t, &n)) return false;
        }
        if (!(t >= 0.0f)) g_t_neg++;
        const V3 p_hit = r_lens.o + r_lens.d * t;
        const Float r2 = p_hit.x * p_hit.x + p_hit.y * p_hit.y;
        if (r2 > element.aperture_radius * element.aperture_radius) return false;
        r_lens.o = p_hit;
        if (!is_stop) {
            V3 w{0.0f, 0.0f, 0.0f};
            const Float eta_i = element.eta;
            const Float eta_t = (i > 0 && cam.el[i - 1].eta != 0.0f) ? cam.el[i - 1].eta : 1.0f;
            if (!refract(normalize(-r_lens.d), n, eta_i / eta_t, &w)) return false;
            r_lens.d = w;
        }
    }
    if (r_out) *r_out = transform_ray(SCALE_Z, r_lens);
    return true;
}
static inline bool trace_lenses_from_scene(const Camera& cam, const Ray& r_camera, Ray* r_out) {   // :366-421
    Float element_z = -cam.lens_front_z();
    Ray r_lens = transform_ray(SCALE_Z, r_camera);
    for (size_t i = 0; i < cam.el.size(); i++) {
        const rspt_lens_element element = cam.el[i];
        Float t = 0.0f;
        V3 n{0.0f, 0.0f, 0.0f};
        const bool is_stop = element.curvature_radius == 0.0f;
        if (is_stop) t = (element_z - r_lens.o.z) / r_lens.d.z;
        else {
            const Float radius = element.curvature_radius;
            const Float z_center = element_z + element.curvature_radius;
            if (!intersect_spherical_element(radius, z_center, r_lens, &t, &n)) return false;
        }
        if (!(t >= 0.0f)) g_t_neg++;
        const V3 p_hit = r_lens.o + r_lens.d * t;
        const Float r2 = p_hit.x * p_hit.x + p_hit.y * p_hit.y;
        if (r2 > element.aperture_radius * element.aperture_radius) return false;
        r_lens.o = p_hit;
        if (!is_stop) {
            V3 wt{0.0f, 0.0f, 0.0f};
            const Float eta_i = (i == 0 || cam.el[i - 1].eta == 0.0f) ? 1.0f : cam.el[i - 1].eta;
            const Float eta_t = cam.el[i].eta != 0.0f ? cam.el[i].eta : 1.0f;
            if (!refract(normalize(-r_lens.d), n, eta_i / eta_t, &wt)) return false;
            r_lens.d = wt;
        }
        element_z += element.thickness;
    }
    if (r_out) *r_out = transform_ray(SCALE_Z, r_lens);
    return true;
}
static inline void compute_cardinal_points(const Ray& r_in, const Ray& r_out, int idx, Float pz[2], Float fz[2]) {   // :431-443
    const Float tf = -r_out.o.x / r_out.d.x;
    fz[idx] = -(r_out.o + r_out.d * tf).z;
    const Float tp = (r_in.o.x - r_out.o.x) / r_out.d.x;
    pz[idx] = -(r_out.o + r_out.d * tp).z;
}
// 0, or which of the two assertions of :465 / :479 fails
static inline int compute_thick_lens_approximation(const Camera& cam, Float pz[2], Float fz[2]) {   // :444-482
    const Float x = 0.001f * cam.diagonal;
    Ray r_scene{V3{x, 0.0f, cam.lens_front_z() + 1.0f}, V3{0.0f, 0.0f, -1.0f}, INF, 0.0f};
    Ray r_film{V3{0, 0, 0}, V3{0, 0, 0}, 0.0f, 0.0f};
    if (!trace_lenses_from_scene(cam, r_scene, &r_film)) return 1;
    compute_cardinal_points(r_scene, r_film, 0, pz, fz);
    r_film.o = V3{x, 0.0f, cam.lens_rear_z() - 1.0f};
    r_film.d = V3{0.0f, 0.0f, 1.0f};
    if (!trace_lenses_from_film(cam, r_film, &r_scene)) return 2;
    compute_cardinal_points(r_film, r_scene, 1, pz, fz);
    return 0;
}
// 0 and *out = the film distance, or 1 / 2 (the thick-lens assertions) or 3 (assert!(c > 0))
static inline int focus_thick_lens(const Camera& cam, Float focus_distance, Float* out) {   // :483-499
    Float pz[2] = {0.0f, 0.0f}, fz[2] = {0.0f, 0.0f};
    if (int e = compute_thick_lens_approximation(cam, pz, fz)) return e;
    const Float f = fz[0] - pz[0];
    const Float z = -focus_distance;
    const Float c = (pz[1] - z - pz[0]) * (pz[1] - z - 4.0f * f - pz[0]);
    if (!(c > 0.0f)) return 3;
    const Float delta = 0.5f * (pz[1] - z + pz[0] - std::sqrt(c));
    *out = cam.el.back().thickness + delta;
    return 0;
}
static inline Bounds2 bound_exit_pupil(const Camera& cam, Float p_film_x0, Float p_film_x1) {   // :573-652
    Bounds2 pupil_bounds;
    const int32_t n_samples = 1024 * 1024;
    int32_t n_exiting_rays = 0;
    const Float rear_radius = cam.rear_element_radius();
    Bounds2 proj_rear_bounds;
    proj_rear_bounds.p_min = P2{-1.5f * rear_radius, -1.5f * rear_radius};
    proj_rear_bounds.p_max = P2{1.5f * rear_radius, 1.5f * rear_radius};
    for (int32_t i = 0; i < n_samples; i++) {
        const V3 p_film{lerp(((Float)i + 0.5f) / (Float)n_samples, p_film_x0, p_film_x1), 0.0f, 0.0f};
        const Float u[2] = {radical_inverse(0, (uint64_t)i), radical_inverse(1, (uint64_t)i)};
        const V3 p_rear{lerp(u[0], proj_rear_bounds.p_min.x, proj_rear_bounds.p_max.x), lerp(u[1], proj_rear_bounds.p_min.y, proj_rear_bounds.p_max.y), cam.lens_rear_z()};
        if (pupil_bounds.inside(P2{p_rear.x, p_rear.y}) || trace_lenses_from_film(cam, Ray{p_film, p_rear - p_film, INF, 0.0f}, nullptr)) {
            pupil_bounds.p_min = P2{std::fmin(pupil_bounds.p_min.x, p_rear.x), std::fmin(pupil_bounds.p_min.y, p_rear.y)};   // bnd2_union_pnt2
            pupil_bounds.p_max = P2{std::fmax(pupil_bounds.p_max.x, p_rear.x), std::fmax(pupil_bounds.p_max.y, p_rear.y)};
            n_exiting_rays++;
        }
    }
    if (n_exiting_rays == 0) return proj_rear_bounds;
    const P2 diag{proj_rear_bounds.p_max.x - proj_rear_bounds.p_min.x, proj_rear_bounds.p_max.y - proj_rear_bounds.p_min.y};
    const Float delta = 2.0f * std::sqrt(diag.x * diag.x + diag.y * diag.y) / std::sqrt((Float)n_samples);
    pupil_bounds.p_min = P2{pupil_bounds.p_min.x - delta, pupil_bounds.p_min.y - delta};   // bnd2_expand
    pupil_bounds.p_max = P2{pupil_bounds.p_max.x + delta, pupil_bounds.p_max.y + delta};
    return pupil_bounds;
}
// RealisticCamera::new (:50-144): 0, or the assertion that fails (1, 2, 3 as focus_thick_lens)
static inline int setup(const float* lens_data, uint32_t n, Float aperture_diameter, Float focus_distance, Float film_diagonal_mm, uint32_t n_bounds, int threads, Camera* cam) {
    cam->el.clear();
    for (uint32_t i = 0; i < 4 * n; i += 4) {
        Float diameter = lens_data[i + 3];
        if (lens_data[i] == 0.0f) {
            if (aperture_diameter > lens_data[i + 3]) { /* "Specified aperture diameter ... is greater than maximum possible ...  Clamping it." */ }
            else diameter = aperture_diameter;
        }
        cam->el.push_back(rspt_lens_element{lens_data[i] * 0.001f, lens_data[i + 1] * 0.001f, lens_data[i + 2], diameter * 0.001f / 2.0f});
    }
    cam->diagonal = film_diagonal_mm * 0.001f;   // Film::new, film.rs:214
    Float thick = 0.0f;
    if (int e = focus_thick_lens(*cam, focus_distance, &thick)) return e;
    cam->el.back().thickness = thick;
    cam->pupil.assign(n_bounds, Bounds2{});
    std::atomic<uint32_t> next{0};
    auto worker = [&]() {
        for (;;) {
            const uint32_t i = next.fetch_add(1);
            if (i >= n_bounds) break;
            const Float r0 = (Float)i / (Float)n_bounds * cam->diagonal / 2.0f;
            const Float r1 = (Float)(i + 1) / (Float)n_bounds * cam->diagonal / 2.0f;
            cam->pupil[i] = bound_exit_pupil(*cam, r0, r1);
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < threads; t++) th.emplace_back(worker);
    worker();
    for (auto& t : th) t.join();
    return 0;
}
static inline Camera camera_of(const rspt_render_desc& rd) {
    Camera cam;
    cam.el.assign(rd.lens_elements, rd.lens_elements + rd.n_lens_elements);
    for (uint32_t i = 0; i < rd.n_exit_pupil_bounds; i++) {
        Bounds2 b;
        b.p_min = P2{rd.exit_pupil_bounds[4 * i], rd.exit_pupil_bounds[4 * i + 1]};
        b.p_max = P2{rd.exit_pupil_bounds[4 * i + 2], rd.exit_pupil_bounds[4 * i + 3]};
        cam.pupil.push_back(b);
    }
    cam.diagonal = rd.film_diagonal;
    cam.res[0] = rd.full_res[0]; cam.res[1] = rd.full_res[1];
    cam.shutter_open = rd.shutter_open; cam.shutter_close = rd.shutter_close;
    cam.simple_weighting = rd.lens_simple_weighting != 0;
    return cam;
}
static inline V3 sample_exit_pupil(const Camera& cam, P2 p_film, P2 lens_sample, Float* sample_bounds_area) {   // :656-688
    const Float r_film = std::sqrt(p_film.x * p_film.x + p_film.y * p_film.y);
    size_t r_index = (size_t)f2usize(std::floor(r_film / (cam.diagonal / 2.0f) * (Float)cam.pupil.size()));
    r_index = std::min(cam.pupil.size() - 1, r_index);
    const Bounds2 pupil_bounds = cam.pupil[r_index];
    *sample_bounds_area = pupil_bounds.area();
    const P2 p_lens = pupil_bounds.lerp2(lens_sample);
    const Float sin_theta = r_film != 0.0f ? p_film.y / r_film : 0.0f;
    const Float cos_theta = r_film != 0.0f ? p_film.x / r_film : 1.0f;
    return V3{cos_theta * p_lens.x - sin_theta * p_lens.y, sin_theta * p_lens.x + cos_theta * p_lens.y, cam.lens_rear_z()};
}
static inline Bounds2 physical_extent(const Camera& cam) {   // Film::get_physical_extent, film.rs:293-307
    const Float aspect = (Float)cam.res[1] / (Float)cam.res[0];
    const Float x = std::sqrt(cam.diagonal * cam.diagonal / (1.0f + aspect * aspect));
    const Float y = aspect * x;
    Bounds2 b;
    b.p_min = P2{-x / 2.0f, -y / 2.0f};
    b.p_max = P2{x / 2.0f, y / 2.0f};
    return b;
}
// generate_ray (:198-251); `ray` is written only when the trace succeeds
static inline Float generate_ray(const Camera& cam, const AnimatedTransform& c2w, P2 s_film, Float s_time, P2 s_lens, Ray* ray) {
    const P2 s{s_film.x / (Float)cam.res[0], s_film.y / (Float)cam.res[1]};
    const P2 p_film2 = physical_extent(cam).lerp2(s);
    const V3 p_film{-p_film2.x, p_film2.y, 0.0f};
    Float exit_pupil_bounds_area = 0.0f;
    const V3 p_rear = sample_exit_pupil(cam, P2{p_film.x, p_film.y}, s_lens, &exit_pupil_bounds_area);
    const Ray r_film{p_film, p_rear - p_film, INF, lerp(s_time, cam.shutter_open, cam.shutter_close)};
    if (!trace_lenses_from_film(cam, r_film, ray)) return 0.0f;
    *ray = c2w.transform_ray(*ray);
    ray->d = normalize(ray->d);
    const Float cos_theta = normalize(r_film.d).z;
    const Float cos_2_theta = cos_theta * cos_theta;
    const Float cos_4_theta = cos_2_theta * cos_2_theta;
    if (cam.simple_weighting) return cos_4_theta * exit_pupil_bounds_area / cam.pupil[0].area();
    return (cam.shutter_close - cam.shutter_open) * (cos_4_theta * exit_pupil_bounds_area) / (cam.lens_rear_z() * cam.lens_rear_z());
}
static inline Ray default_ray() { return Ray{V3{0, 0, 0}, V3{0, 0, 0}, 0.0f, 0.0f}; }   // #[derive(Default)]
// generate_ray_differential (:693-735).  *arm: 0 the primary ray is vignetted, 1 clean, 2 x retried with -0.05, 3 y retried (x possibly too),
// 4 dead by both x shifts, 5 dead by both y shifts
static inline Float generate_ray_differential(const Camera& cam, const AnimatedTransform& c2w, P2 s_film, Float s_time, P2 s_lens, Ray* ray, int* arm) {
    int a = 1;
    const Float wt = generate_ray(cam, c2w, s_film, s_time, s_lens, ray);
    if (wt == 0.0f) { if (arm) *arm = 0; return 0.0f; }
    V3 rx_o{0, 0, 0}, rx_d{0, 0, 0}, ry_o{0, 0, 0}, ry_d{0, 0, 0};
    const Float eps_values[2] = {0.05f, -0.05f};
    Float wtx = 0.0f;
    for (int e = 0; e < 2; e++) {
        const Float eps = eps_values[e];
        if (e == 1) a = 2;
        Ray rx = default_ray();
        wtx = generate_ray(cam, c2w, P2{s_film.x + eps, s_film.y}, s_time, s_lens, &rx);
        rx_o = ray->o + (rx.o - ray->o) / eps;
        rx_d = ray->d + (rx.d - ray->d) / eps;
        if (wtx != 0.0f) break;
    }
    if (wtx == 0.0f) { if (arm) *arm = 4; return 0.0f; }
    Float wty = 0.0f;
    for (int e = 0; e < 2; e++) {
        const Float eps = eps_values[e];
        if (e == 1) a = 3;
        Ray ry = default_ray();
        wty = generate_ray(cam, c2w, P2{s_film.x, s_film.y + eps}, s_time, s_lens, &ry);
        ry_o = ray->o + (ry.o - ray->o) / eps;
        ry_d = ray->d + (ry.d - ray->d) / eps;
        if (wty != 0.0f) break;
    }
    if (wty == 0.0f) { if (arm) *arm = 5; return 0.0f; }
    ray->has_diff = true;
    ray->rx_o = rx_o; ray->rx_d = rx_d; ray->ry_o = ry_o; ray->ry_d = ry_d;
    if (arm) *arm = a;
    return wt;
}

// ---- (b) orc::render (oracle/orc_render.hpp) with the camera chosen by camera_kind, a real ray_weight and `if ray_weight > 0 { li }` ----
static inline void render(const Scene& scene, const rspt_render_desc& rd, int num_threads, float* film_xyzw, float* li_rgb, float* weights, int ext_integrator,
                          int direct_strategy, const int32_t* n_light_samples, bool zero_diff) {
    scene.prepare_media();
    RenderCtx cx;
    cx.scene = &scene; cx.rd = &rd;
    cx.ext_integrator = ext_integrator; cx.direct_strategy = direct_strategy;
    for (uint32_t i = 0; i < scene.d.n_lights; i++) cx.n_light_samples.push_back(n_light_samples ? n_light_samples[i] : 1);
    light_distrib_init(cx);
    const int32_t* sb = rd.sample_bounds;
    int32_t ext_x = sb[2] - sb[0], ext_y = sb[3] - sb[1];
    int32_t ts = (int32_t)rd.tile_size;
    int32_t ntx = (ext_x + ts - 1) / ts, nty = (ext_y + ts - 1) / ts;
    std::vector<std::pair<uint32_t, uint32_t>> blocks;
    for (int32_t i = 0; i < ntx * nty; i++) blocks.push_back({(uint32_t)(i % ntx), (uint32_t)(i / ntx)});
    std::stable_sort(blocks.begin(), blocks.end(), [](auto a, auto b) { return morton2(a.first, a.second) < morton2(b.first, b.second); });
    std::vector<size_t> mine;
    uint32_t chunk = rd.tile_chunk ? rd.tile_chunk : 1, sc_ = rd.shard_count ? rd.shard_count : 1;
    for (size_t i = 0; i < blocks.size(); i++) if ((i / chunk) % sc_ == rd.shard_index) mine.push_back(i);
    std::vector<FilmTile> tiles(mine.size());
    std::atomic<size_t> next{0};
    int cw = rd.crop_px[2] - rd.crop_px[0], ch = rd.crop_px[3] - rd.crop_px[1];
    std::vector<Counters> tc((size_t)std::max(1, num_threads));
    const AnimatedTransform cam_c2w = camera_animation(rd);
    const bool realistic = rd.camera_kind == RSPT_CAMERA_REALISTIC;
    const Camera lens_cam = realistic ? camera_of(rd) : Camera{};
    auto worker = [&](int tid) {
        Sampler sampler(rd);
        if (rd.integrator == RSPT_INTEGRATOR_AO && ext_integrator == ORC_INTEGRATOR_FROM_DESC) sampler.request_2d_array((int32_t)rd.ao_n_samples);
        if (ext_integrator == ORC_INTEGRATOR_DIRECT && direct_strategy == ORC_DIRECT_SAMPLE_ALL)
            for (uint32_t i = 0; i < rd.max_depth; i++)
                for (uint32_t j = 0; j < scene.d.n_lights; j++) { sampler.request_2d_array(cx.n_light_samples[j]); sampler.request_2d_array(cx.n_light_samples[j]); }
        Counters& c = tc[tid];
        for (;;) {
            size_t k = next.fetch_add(1);
            if (k >= mine.size()) break;
            auto blk = blocks[mine[k]];
            int32_t x0 = sb[0] + (int32_t)blk.first * ts, x1 = std::min(x0 + ts, sb[2]);
            int32_t y0 = sb[1] + (int32_t)blk.second * ts, y1 = std::min(y0 + ts, sb[3]);
            int32_t tb[4] = {x0, y0, x1, y1};
            FilmTile ft = get_film_tile(rd, tb);
            sampler.reseed((uint64_t)(int64_t)(int32_t)((int32_t)blk.second * ntx + (int32_t)blk.first));
            for (int32_t py = y0; py < y1; py++)
                for (int32_t px = x0; px < x1; px++) {
                    sampler.start_pixel(px, py);
                    if (!(px >= sb[0] && px < sb[2] && py >= sb[1] && py < sb[3])) continue;
                    bool done = false;
                    while (!done) {
                        P2 f2 = sampler.get_2d();
                        P2 p_film{(Float)px + f2.x, (Float)py + f2.y};
                        Float time_s = sampler.get_1d();
                        P2 p_lens = sampler.get_2d();
                        Ray ray = default_ray();
                        Float ray_weight = 1.0f;
                        if (realistic) ray_weight = generate_ray_differential(lens_cam, cam_c2w, p_film, time_s, p_lens, &ray, nullptr);
                        else ray = camera_ray(rd, cam_c2w, p_film, time_s, p_lens);
                        if (zero_diff) ray.has_diff = false;
                        ray.scale_differentials(1.0f / std::sqrt((Float)rd.spp));
                        if (rd.sample_count && ((uint64_t)sampler.cur_sample() < rd.sample_begin || (uint64_t)sampler.cur_sample() >= rd.sample_begin + rd.sample_count)) {
                            done = !sampler.start_next_sample();
                            continue;
                        }
                        Spec l(0.0f);
                        if (ray_weight > 0.0f)
                            l = (ext_integrator == ORC_INTEGRATOR_DIRECT && g_direct_li_override) ? g_direct_li_override(cx, ray, sampler, &c)
                                : ext_integrator != ORC_INTEGRATOR_FROM_DESC ? recursive_li(cx, ray, sampler, 0, &c)
                                : rd.integrator == RSPT_INTEGRATOR_AO       ? (g_ao_li_override ? g_ao_li_override(cx, ray, sampler, &c) : ao_li(cx, ray, sampler, &c))
                                : rd.integrator == RSPT_INTEGRATOR_VOLPATH  ? volpath_li(cx, ray, sampler, &c)
                                : g_li_override                             ? g_li_override(cx, ray, sampler, &c)
                                                                            : path_li(cx, ray, sampler, &c);
                        c.samples++;
                        if (l.has_nans()) { l = Spec(0.0f); c.nan_samples++; }
                        if (px >= rd.crop_px[0] && px < rd.crop_px[2] && py >= rd.crop_px[1] && py < rd.crop_px[3]) {
                            size_t pix = (size_t)(py - rd.crop_px[1]) * cw + (size_t)(px - rd.crop_px[0]);
                            size_t at = pix * (size_t)rd.spp + (size_t)sampler.cur_sample();
                            if (li_rgb) { float* o = li_rgb + at * 3; o[0] = l.c[0]; o[1] = l.c[1]; o[2] = l.c[2]; }
                            if (weights) weights[at] = ray_weight;
                        }
                        ft.add_sample(rd, p_film, l, ray_weight);
                        done = !sampler.start_next_sample();
                    }
                }
            tiles[k] = std::move(ft);
        }
    };
    if (num_threads <= 1) worker(0);
    else {
        std::vector<std::thread> th;
        for (int i = 0; i < num_threads; i++) th.emplace_back(worker, i);
        for (auto& t : th) t.join();
    }
    if (film_xyzw) {
        std::memset(film_xyzw, 0, sizeof(float) * 4 * (size_t)cw * ch);
        for (const FilmTile& t : tiles) merge_film_tile(rd, t, film_xyzw);
    }
}

}  // namespace real
}  // namespace orc

// ---- (c) ----
extern "C" {
// ext_integrator / direct_strategy / n_light_samples as orc_render_integrator takes them (ORC_INTEGRATOR_FROM_DESC = the desc's path / ao / volpath); film_xyzw
// (npix, 4), li_rgb (npix * spp * 3) and weights (npix * spp: every sample's ray weight), each may be NULL.  zero_diff: the camera ray is handed to li without
// its differentials.  camera_kind 0 (the oracle's perspective camera, weight 1) or 3.
int real_render(const rspt_scene_desc* sd, const rspt_render_desc* rd, int num_threads, float* film_xyzw, float* li_rgb, float* weights, int ext_integrator,
                int direct_strategy, const int32_t* n_light_samples, int zero_diff) {
    if (!sd || !rd || (rd->camera_kind != RSPT_CAMERA_PERSPECTIVE && rd->camera_kind != RSPT_CAMERA_REALISTIC)) return -1;
#ifdef CAM_LI_SPHERES
    orc::g_li_override = orc::sphr::path_li;
    orc::g_ao_li_override = orc::sphr::ao_li;
#endif
    orc::Scene sc{*sd};
    orc::real::render(sc, *rd, num_threads, film_xyzw, li_rgb, weights, ext_integrator, direct_strategy, n_light_samples, zero_diff != 0);
#ifdef CAM_LI_SPHERES
    orc::g_li_override = nullptr;
    orc::g_ao_li_override = nullptr;
#endif
    return 0;
}
// generate_ray_differential over n CameraSamples (n x 5: p_film.x, p_film.y, time, p_lens.x, p_lens.y) -> out n x 22 (weight, o, d, t_max, time, rx_o, rx_d,
// ry_o, ry_d, has_diff: rspt_camera_rays' layout, differentials unscaled and zero where the weight is 0) and arms[n] (see generate_ray_differential)
void real_rays(const rspt_render_desc* rd, const float* samples, uint64_t n, float* out, int32_t* arms) {
    const orc::real::Camera cam = orc::real::camera_of(*rd);
    const orc::AnimatedTransform c2w = orc::camera_animation(*rd);
    for (uint64_t i = 0; i < n; i++) {
        const float* s = samples + 5 * i;
        orc::Ray ray = orc::real::default_ray();
        int arm = 0;
        const float w = orc::real::generate_ray_differential(cam, c2w, orc::P2{s[0], s[1]}, s[2], orc::P2{s[3], s[4]}, &ray, &arm);
        float* o = out + 22 * i;
        o[0] = w; o[1] = ray.o.x; o[2] = ray.o.y; o[3] = ray.o.z; o[4] = ray.d.x; o[5] = ray.d.y; o[6] = ray.d.z; o[7] = ray.t_max; o[8] = ray.time;
        const orc::V3 v[4] = {ray.rx_o, ray.rx_d, ray.ry_o, ray.ry_d};
        for (int j = 0; j < 4; j++) { o[9 + 3 * j] = v[j].x; o[10 + 3 * j] = v[j].y; o[11 + 3 * j] = v[j].z; }
        o[21] = ray.has_diff ? 1.0f : 0.0f;
        if (arms) arms[i] = arm;
    }
}
// RealisticCamera::new's state: 0, or 1 / 2 ("Unable to trace ray from scene to film / from film to scene for thick lens approximation"), 3 ("Coefficient must be positive")
int real_setup(const float* lens_data, uint32_t n_elements, float aperture_diameter_mm, float focus_distance, float film_diagonal_mm, uint32_t n_bounds,
               rspt_lens_element* elements_out, float* bounds_out, int threads) {
    orc::real::Camera cam;
    if (int e = orc::real::setup(lens_data, n_elements, aperture_diameter_mm, focus_distance, film_diagonal_mm, n_bounds, threads, &cam)) return e;
    std::memcpy(elements_out, cam.el.data(), n_elements * sizeof(rspt_lens_element));
    for (uint32_t i = 0; i < n_bounds; i++) {
        bounds_out[4 * i] = cam.pupil[i].p_min.x; bounds_out[4 * i + 1] = cam.pupil[i].p_min.y;
        bounds_out[4 * i + 2] = cam.pupil[i].p_max.x; bounds_out[4 * i + 3] = cam.pupil[i].p_max.y;
    }
    return 0;
}
// trace_lenses_from_film for one camera-space ray over an element table (metres, as the desc takes it): 1 and out = o, d, t_max (7 floats), or 0
int real_trace_from_film(const rspt_lens_element* elements, uint32_t n, const float o[3], const float d[3], float out[7]) {
    orc::real::Camera cam;
    cam.el.assign(elements, elements + n);
    orc::Ray r = orc::real::default_ray();
    if (!orc::real::trace_lenses_from_film(cam, orc::Ray{orc::V3{o[0], o[1], o[2]}, orc::V3{d[0], d[1], d[2]}, orc::INF, 0.0f}, &r)) return 0;
    out[0] = r.o.x; out[1] = r.o.y; out[2] = r.o.z; out[3] = r.d.x; out[4] = r.d.y; out[5] = r.d.z; out[6] = r.t_max;
    return 1;
}
// trace_lenses_from_scene, the same way
int real_trace_from_scene(const rspt_lens_element* elements, uint32_t n, const float o[3], const float d[3], float out[7]) {
    orc::real::Camera cam;
    cam.el.assign(elements, elements + n);
    orc::Ray r = orc::real::default_ray();
    if (!orc::real::trace_lenses_from_scene(cam, orc::Ray{orc::V3{o[0], o[1], o[2]}, orc::V3{d[0], d[1], d[2]}, orc::INF, 0.0f}, &r)) return 0;
    out[0] = r.o.x; out[1] = r.o.y; out[2] = r.o.z; out[3] = r.d.x; out[4] = r.d.y; out[5] = r.d.z; out[6] = r.t_max;
    return 1;
}
// compute_thick_lens_approximation over an element table and a film diagonal in metres: pz[2], fz[2]; 0 or the failing assertion
int real_cardinal_points(const rspt_lens_element* elements, uint32_t n, float film_diagonal, float pz[2], float fz[2]) {
    orc::real::Camera cam;
    cam.el.assign(elements, elements + n);
    cam.diagonal = film_diagonal;
    return orc::real::compute_thick_lens_approximation(cam, pz, fz);
}
uint64_t real_t_neg_count(void) { return orc::real::g_t_neg.load(); }
// Sampler::get_camera_sample of sample s of pixel (px, py) as the tile loop draws it: out = p_film.x, p_film.y, time, p_lens.x, p_lens.y
void real_sample(const rspt_render_desc* rd, int32_t px, int32_t py, int64_t s, float out[5]) {
    orc::Sampler sampler(*rd);
    sampler.start_pixel(px, py);
    for (int64_t i = 0; i < s; i++) sampler.start_next_sample();
    const orc::P2 f2 = sampler.get_2d();
    out[0] = (orc::Float)px + f2.x; out[1] = (orc::Float)py + f2.y;
    out[2] = sampler.get_1d();
    const orc::P2 l = sampler.get_2d();
    out[3] = l.x; out[4] = l.y;
}
}
