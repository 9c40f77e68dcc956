// The CPU yardstick of the orthographic and environment cameras (ABI 25).  The oracle knows the perspective camera only and `li` never sees p_film, so no
// li override can put another camera under orc::render.  This file therefore holds
//   (a) OrthographicCamera::generate_ray_differential (src/cameras/orthographic.rs:150-235) and EnvironmentCamera::generate_ray_differential
//       (src/cameras/environment.rs:92-116), written from the reference's text over the oracle's leaf functions;
//   (b) cam_render: orc::render's tile loop (SamplerIntegrator::render, src/core/integrator.rs:70-220) restated line for line — the same sampler calls in
//       the same order, scale_differentials, the NaN rule, film tiles, Morton merge — with the camera chosen by rd->camera_kind and the oracle's own
//       path_li / ao_li / volpath_li / recursive_li (or the g_*_override pointers, as orc::render honours them);
//   (c) a small extern "C" surface.
// tests/test_camera_host.py first holds cam_render with camera_kind = 0 to orc::render bit for bit (film and every sample's li), then the two new
// cameras to known answers; tests/test_gpu_cameras.py holds rspt_render to cam_render.
// Built by the tests: g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared -I oracle -I include -I tests.
// -DCAM_LI_SPHERES (with tests/sphere_render_restated.cpp linked in): cam_render installs that file's li restatements, as its own render entry does around
// orc::render.  (tests/maplight_restated.cpp keeps its li and the view it needs private to its own entry, so map lights have no such switch.)
#include "orc_render.hpp"

namespace orc {
#ifdef CAM_LI_SPHERES
namespace sphr { Spec path_li(RenderCtx& cx, const Ray& r, Sampler& sampler, Counters* c); Spec ao_li(RenderCtx& cx, const Ray& ray, Sampler& sampler, Counters* c); }
#endif
namespace cam {

// ---- (a) ----
// OrthographicCamera::new's dx_camera / dy_camera (orthographic.rs:73-82): the VECTOR transform of the raster axes
static inline Ray ortho_camera_ray_in(const rspt_render_desc& rd, P2 p_film_, Float time_s, P2 p_lens_) {
    const V3 dx_camera = transform_vector(rd.raster_to_camera, V3{1.0f, 0.0f, 0.0f});
    const V3 dy_camera = transform_vector(rd.raster_to_camera, V3{0.0f, 1.0f, 0.0f});
    const V3 p_film{p_film_.x, p_film_.y, 0.0f};                                       // :153-157
    const V3 p_camera = transform_point(rd.raster_to_camera, p_film);                // :158
    Ray ray{p_camera, V3{0.0f, 0.0f, 1.0f}, INF, lerp(time_s, rd.shutter_open, rd.shutter_close)};   // :159-170
    if (rd.lens_radius > 0.0f) {                                                     // :172-185
        const P2 d = concentric_sample_disk(p_lens_);
        const P2 p_lens{d.x * rd.lens_radius, d.y * rd.lens_radius};
        const Float ft = rd.focal_distance / ray.d.z;
        const V3 p_focus = ray.o + ray.d * ft;                                       // ray.position(ft)
        ray.o = V3{p_lens.x, p_lens.y, 0.0f};
        ray.d = normalize(p_focus - ray.o);
    }
    ray.has_diff = true;
    if (rd.lens_radius > 0.0f) {                                                     // :187-217
        const P2 d = concentric_sample_disk(p_lens_);
        const P2 p_lens{d.x * rd.lens_radius, d.y * rd.lens_radius};
        const Float ft = rd.focal_distance / ray.d.z;                                // ray.d: already the lens ray's direction
        const V3 p_focus = p_camera + dx_camera + (V3{0.0f, 0.0f, 1.0f} * ft);       // dy_camera is not used: ry == rx
        ray.rx_o = V3{p_lens.x, p_lens.y, 0.0f};
        ray.ry_o = V3{p_lens.x, p_lens.y, 0.0f};
        ray.rx_d = normalize(p_focus - ray.rx_o);
        ray.ry_d = normalize(p_focus - ray.ry_o);
    } else {                                                                         // :218-226
        ray.rx_o = ray.o + dx_camera;
        ray.ry_o = ray.o + dy_camera;
        ray.rx_d = ray.d;
        ray.ry_d = ray.d;
    }
    return ray;
}
static inline Ray environment_camera_ray_in(const rspt_render_desc& rd, P2 p_film, Float time_s) {
    const Float theta = PI * p_film.y / (Float)rd.full_res[1];                       // :93
    const Float phi = 2.0f * PI * p_film.x / (Float)rd.full_res[0];                  // :94
    const V3 dir{std::sin(theta) * std::cos(phi), std::cos(theta), std::sin(theta) * std::sin(phi)};   // :95-99
    return Ray{V3{0.0f, 0.0f, 0.0f}, dir, INF, lerp(time_s, rd.shutter_open, rd.shutter_close)};       // :100-107: differential: None
}
static inline Ray ortho_camera_ray(const rspt_render_desc& rd, const AnimatedTransform& c2w, P2 p_film, Float time_s, P2 p_lens) {
    return c2w.transform_ray(ortho_camera_ray_in(rd, p_film, time_s, p_lens));       // :233
}
static inline Ray environment_camera_ray(const rspt_render_desc& rd, const AnimatedTransform& c2w, P2 p_film, Float time_s) {
    return c2w.transform_ray(environment_camera_ray_in(rd, p_film, time_s));         // :114
}
static inline Ray any_camera_ray(const rspt_render_desc& rd, const AnimatedTransform& c2w, P2 p_film, Float time_s, P2 p_lens) {
    return rd.camera_kind == RSPT_CAMERA_ORTHOGRAPHIC  ? ortho_camera_ray(rd, c2w, p_film, time_s, p_lens)
           : rd.camera_kind == RSPT_CAMERA_ENVIRONMENT ? environment_camera_ray(rd, c2w, p_film, time_s)
                                                       : camera_ray(rd, c2w, p_film, time_s, p_lens);
}

// ---- (b) orc::render (oracle/orc_render.hpp) with any_camera_ray in the place of camera_ray ----
// zero_diff: the camera ray is handed to li WITHOUT its differentials (what the environment camera does) — the switch the texture cases use to show that
// they can tell the difference
static inline void render(const Scene& scene, const rspt_render_desc& rd, int num_threads, float* film_xyzw, float* li_rgb, int ext_integrator, int direct_strategy,
                          const int32_t* n_light_samples, bool zero_diff) {
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
                        Ray ray = any_camera_ray(rd, cam_c2w, p_film, time_s, p_lens);
                        if (zero_diff) ray.has_diff = false;
                        ray.scale_differentials(1.0f / std::sqrt((Float)rd.spp));
                        Float ray_weight = 1.0f;
                        if (rd.sample_count && ((uint64_t)sampler.cur_sample() < rd.sample_begin || (uint64_t)sampler.cur_sample() >= rd.sample_begin + rd.sample_count)) {
                            done = !sampler.start_next_sample();
                            continue;
                        }
                        Spec l = (ext_integrator == ORC_INTEGRATOR_DIRECT && g_direct_li_override) ? g_direct_li_override(cx, ray, sampler, &c)
                                 : ext_integrator != ORC_INTEGRATOR_FROM_DESC ? recursive_li(cx, ray, sampler, 0, &c)
                                 : rd.integrator == RSPT_INTEGRATOR_AO       ? (g_ao_li_override ? g_ao_li_override(cx, ray, sampler, &c) : ao_li(cx, ray, sampler, &c))
                                 : rd.integrator == RSPT_INTEGRATOR_VOLPATH  ? volpath_li(cx, ray, sampler, &c)
                                 : g_li_override                             ? g_li_override(cx, ray, sampler, &c)
                                                                             : path_li(cx, ray, sampler, &c);
                        c.samples++;
                        if (l.has_nans()) { l = Spec(0.0f); c.nan_samples++; }
                        if (li_rgb && px >= rd.crop_px[0] && px < rd.crop_px[2] && py >= rd.crop_px[1] && py < rd.crop_px[3]) {
                            size_t pix = (size_t)(py - rd.crop_px[1]) * cw + (size_t)(px - rd.crop_px[0]);
                            float* o = li_rgb + (pix * (size_t)rd.spp + (size_t)sampler.cur_sample()) * 3;
                            o[0] = l.c[0]; o[1] = l.c[1]; o[2] = l.c[2];
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

static inline void put3(float* out, V3 v) { out[0] = v.x; out[1] = v.y; out[2] = v.z; }
static inline void put_ray(const Ray& r, float out[21]) {
    put3(out, r.o); put3(out + 3, r.d);
    out[6] = r.t_max; out[7] = r.time; out[8] = r.has_diff ? 1.0f : 0.0f;
    put3(out + 9, r.rx_o); put3(out + 12, r.rx_d); put3(out + 15, r.ry_o); put3(out + 18, r.ry_d);
}

}  // namespace cam
}  // namespace orc

// ---- (c) ----
extern "C" {
// ext_integrator / direct_strategy / n_light_samples as orc_render_integrator takes them (ORC_INTEGRATOR_FROM_DESC = the desc's path / ao / volpath);
// film_xyzw (npix, 4) and li_rgb (npix * spp * 3, or NULL) as orc_render fills them.  zero_diff: see orc::cam::render.
int cam_render(const rspt_scene_desc* sd, const rspt_render_desc* rd, int num_threads, float* film_xyzw, float* li_rgb, int ext_integrator, int direct_strategy,
               const int32_t* n_light_samples, int zero_diff) {
    if (!sd || !rd || rd->camera_kind > RSPT_CAMERA_ENVIRONMENT) return -1;
#ifdef CAM_LI_SPHERES
    orc::g_li_override = orc::sphr::path_li;
    orc::g_ao_li_override = orc::sphr::ao_li;
#endif
    orc::Scene sc{*sd};
    orc::cam::render(sc, *rd, num_threads, film_xyzw, li_rgb, ext_integrator, direct_strategy, n_light_samples, zero_diff != 0);
#ifdef CAM_LI_SPHERES
    orc::g_li_override = nullptr;
    orc::g_ao_li_override = nullptr;
#endif
    return 0;
}
// The camera's ray for one CameraSample (p_film, time, p_lens), before scale_differentials: out = o, d, t_max, time, has_diff, rx_o, rx_d, ry_o, ry_d (21 floats)
void cam_ray(const rspt_render_desc* rd, const float p_film[2], float time, const float p_lens[2], float out[21]) {
    orc::cam::put_ray(orc::cam::any_camera_ray(*rd, orc::camera_animation(*rd), orc::P2{p_film[0], p_film[1]}, time, orc::P2{p_lens[0], p_lens[1]}), out);
}
// the same ray in camera space: what generate_ray_differential holds before camera_to_world.transform_ray (orthographic and environment only)
int cam_ray_camera_space(const rspt_render_desc* rd, const float p_film[2], float time, const float p_lens[2], float out[21]) {
    if (rd->camera_kind == RSPT_CAMERA_ORTHOGRAPHIC) orc::cam::put_ray(orc::cam::ortho_camera_ray_in(*rd, orc::P2{p_film[0], p_film[1]}, time, orc::P2{p_lens[0], p_lens[1]}), out);
    else if (rd->camera_kind == RSPT_CAMERA_ENVIRONMENT) orc::cam::put_ray(orc::cam::environment_camera_ray_in(*rd, orc::P2{p_film[0], p_film[1]}, time), out);
    else return -1;
    return 0;
}
// Sampler::get_camera_sample of sample s of pixel (px, py), as the tile loop draws it (Sobol' / Halton: a function of the pixel and the sample index alone):
// out = p_film.x, p_film.y, time, p_lens.x, p_lens.y
void cam_sample(const rspt_render_desc* rd, int32_t px, int32_t py, int64_t s, float out[5]) {
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
