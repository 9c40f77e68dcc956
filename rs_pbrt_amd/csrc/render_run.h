// The state of one rspt_render call (RenderRun): what its setup steps compute and its schedules (render_schedules.h, render_tile_serial.h) read.
// Host code of librspt.hip, included there once inside its anonymous namespace.
#ifndef RSPT_DL_WAVES_DEFAULT
#define RSPT_DL_WAVES_DEFAULT 0
#endif
constexpr int RSPT_DL_RETRY_LANE = -1000;   // batch_direct -> the batch loop: redo this batch with the per-lane form (never leaves render_impl)
struct DevTemps { std::vector<void*> p; ~DevTemps() { for (void* q : p) (void)hipFree(q); } };   // frees a render's temporary device allocations when it leaves, early error returns included

struct RenderRun {
    rspt_scene_s* s;
    const rspt_render_desc* d; rspt_render_desc wd;   // the caller's desc, or `wd`: whitted's, rewritten for directlighting's machinery
    RenderRun(rspt_scene_s* s_, const rspt_render_desc* d_) : s(s_), d(d_) {}  RenderRun(const RenderRun&) = delete;   // (d may point at wd)
    // validate(): integrator, sampler, sample range, shard
    bool whitted = false, multi_lobes = true, halton = false, sobol = false, pixel_sampler = false, direct = false, volpath = false, realistic = false;
    const char* dl_name = "directlighting";
    uint64_t smp_begin = 0, smp_end = 0;
    const int32_t* sb = nullptr; const int32_t* cp = nullptr; uint32_t shard_count = 1, chunk = 1;
    // constants(): render constants, sampler tables, light distribution (ld_lazy: on-demand voxels, a mark / build round in front of every shade launch)
    RenderDev rd{}; uint32_t vol_dim_limit = 1024u; LensSystem lens{};   // lens: RSPT_CAMERA_REALISTIC only
    LightDistDev ld; const LightDist* ld_lazy = nullptr;
    // shard_pixels(): tiles of the whole frame, this shard's in Morton order, their pixels (the list outlives its asynchronous upload)
    int32_t ts = 0, ntx = 0; size_t n_blocks = 0, n_pix = 0;
    std::vector<std::pair<uint32_t, uint32_t>> shard_tiles; std::vector<uint32_t> pix;
    // film_buffers(): the film stage's parameters; the temporary device allocations of the whole run
    size_t film_px = 0, sb_px = 0; int film_k = 0; bool film_gather = false; float* li_dev = nullptr;
    DevTemps temps;
    // size_batches(): the wavefront batch, directlighting's form and sizes, the shade kernels (iterations >= move_first of a MOVE render launch shade_move_k)
    size_t cap = 0, pix_per_batch = 1;
    uint32_t ns = 1, ao_n = 1, dl_levels = 0, dl_H = 1, dl_R = 1, move_first = 1;
    bool counters = false, ao = false, dl_lane = false, dl_one_round = false, move = false;
    const char* shade_name = "generic"; ShadeKernel shade_k = nullptr, shade_move_k = nullptr;
    bool sphere_lights = false;   // validate(): the scene holds an emissive sphere and the sphere-light gate is on (rspt_set_sphere_lights): the sphere-light shade sets serve it
    bool quadric_lights = false;  // validate(): a scene with a disk or a cylinder holds an area light on a quadric and the gates it needs are on (rspt_set_quadric_lights): the quadric-light shade sets serve it
    int shade_math = RSPT_SHADE_MATH_EXACT; bool shade_fast = false; char shade_name_fast[48];   // validate(): the mode; size_batches(): whether fast builds serve this render (then shade_name = "<set>-fast")
    // prepare(): the per-lane directlighting forms' arrays, iteration counts, launch geometry, events (kev: per-launch durations, each pair recorded on the
    // stream its kernel runs on — closest-hit, shadow-ray, shade [+ texture])
    float4* dl_tex = nullptr; int32_t* dl_nls = nullptr; uint32_t* dl_words = nullptr; rspt_mat::Built* dl_dyn = nullptr;
    size_t dl_lanes = 0, n_ev = 0;
    uint32_t dl_tex_rows = 0, nominal_iters = 0, max_iters = 0, sob_nd = 0, sob_bits = 0, tgrid = 0, sgrid = 0;
    bool shade_bins = false, bins_first = false, two_streams = false; hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_k0 = nullptr, ev_k1 = nullptr;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> trace_ev, kev[3];
    // run(): running totals; the queue length the null-surface tail of a batch last saw (hinted_grid), 0xffffffff: none
    uint64_t samples = 0, truncated = 0, vol_rays = 0, trace_launches = 0; uint32_t queue_hint = 0xffffffffu;
    int validate(), constants(), shard_pixels(), film_buffers(const float* li_host), size_batches(), prepare(), run(), run_tile_serial();
    int finish(float* film_host, void* film_dev, float* li_host), report(rspt_stats* stats, std::chrono::steady_clock::time_point t_start);
    int film_index(const uint32_t* list, uint32_t n), build_claimed_rows(uint32_t* n_claimed), tune_any(uint32_t batch_n, TraceCall c), tune_camera(uint32_t batch_n, TraceCall c);
    void film_stage(const RenderDev& rd_, const Batch& bt, const PathBuf& fpb, const uint32_t* list);
    int batch_volpath(const Batch& bt, uint32_t& it), batch_direct(const Batch& bt, uint32_t& it), batch_direct_lane(const Batch& bt, uint32_t& it);
    int batch_ao(const Batch& bt, uint32_t& it), batch_path(const Batch& bt, uint32_t& it);
    void ev_open(int kind, int lane) {
        hipEvent_t a = get_event(n_ev++), b = get_event(n_ev++);
        (void)hipEventRecord(a, lane ? g.stream2 : g.stream);
        kev[kind].push_back({a, b});
    }
    void ev_close(int kind, int lane) { (void)hipEventRecord(kev[kind].back().second, lane ? g.stream2 : g.stream); }
    // the schedules' two trace launches: closest hit over a path state's continuation + MIS rays, any hit over its shadow rays; both with this run's counters and queue hint
    TraceCall trace_call(bool any, const PathBuf& P, const uint32_t* queue, const uint32_t* n, uint32_t* cursor, bool count) const {
        TraceCall c; c.queue = queue; c.count_ptr = n; c.cursor = cursor; c.count = count; c.counters = g.totals; c.queue_hint = queue_hint;
        if (any) { c.ra = c.rb = P.ray_sh; c.occ = P.occluded; } else { c.ra = P.ray_cont; c.rb = P.ray_mis; c.oa = P.hit_cont; c.ob = P.hit_mis; }
        return c;
    }
    TraceCall closest_call(const PathBuf& P, const uint32_t* queue, const uint32_t* n, uint32_t* cursor, bool count) const { return trace_call(false, P, queue, n, cursor, count); }
    TraceCall any_call(const PathBuf& P, const uint32_t* queue, const uint32_t* n, uint32_t* cursor, bool count) const { return trace_call(true, P, queue, n, cursor, count); }
};

// The camera part of a render desc (rspt_render and its siblings, rspt_camera_rays): every refusal names camera_kind
int validate_camera(const rspt_render_desc* d) {
    if (d->camera_kind > RSPT_CAMERA_REALISTIC) return fail(RSPT_E_INVALID, "camera_kind %u (0 perspective, 1 orthographic, 2 environment, 3 realistic)", d->camera_kind);
    if (d->camera_kind == RSPT_CAMERA_ENVIRONMENT && (d->full_res[0] <= 0 || d->full_res[1] <= 0)) return fail(RSPT_E_INVALID, "camera_kind environment: full_res must be positive");
    if (d->camera_kind == RSPT_CAMERA_REALISTIC) {
        if (!d->lens_elements || d->n_lens_elements == 0) return fail(RSPT_E_INVALID, "camera_kind realistic: the lens element table is null or empty (rspt_realistic_camera_setup builds it)");
        if (d->n_lens_elements > RSPT_MAX_LENS_ELEMENTS) return fail(RSPT_E_INVALID, "camera_kind realistic: %u lens elements, at most %d are served", d->n_lens_elements, RSPT_MAX_LENS_ELEMENTS);
        if (!d->exit_pupil_bounds || d->n_exit_pupil_bounds == 0) return fail(RSPT_E_INVALID, "camera_kind realistic: the exit pupil bounds table is null or empty (rspt_realistic_camera_setup builds it)");
        if (d->n_exit_pupil_bounds > RSPT_MAX_EXIT_PUPIL_BOUNDS) return fail(RSPT_E_INVALID, "camera_kind realistic: %u exit pupil bounds, at most %d are served", d->n_exit_pupil_bounds, RSPT_MAX_EXIT_PUPIL_BOUNDS);
        if (d->full_res[0] <= 0 || d->full_res[1] <= 0) return fail(RSPT_E_INVALID, "camera_kind realistic: full_res must be positive");
        if (!(d->film_diagonal > 0.0f)) return fail(RSPT_E_INVALID, "camera_kind realistic: film_diagonal must be positive");
    }
    return RSPT_OK;
}
// the lens tables of a realistic camera in device memory (once per render / hook call) and what the tracer reads besides them
int upload_lens(const rspt_render_desc* d, LensSystem* L) {
    int rc;
    if (!g.lens_elements && ((rc = dev_alloc(&g.lens_elements, RSPT_MAX_LENS_ELEMENTS)) || (rc = dev_alloc(&g.lens_bounds, 4 * RSPT_MAX_EXIT_PUPIL_BOUNDS)))) return rc;
    HIP_TRY(hipMemcpyAsync(g.lens_elements, d->lens_elements, d->n_lens_elements * sizeof(rspt_lens_element), hipMemcpyHostToDevice, g.stream));
    HIP_TRY(hipMemcpyAsync(g.lens_bounds, d->exit_pupil_bounds, d->n_exit_pupil_bounds * 4 * sizeof(float), hipMemcpyHostToDevice, g.stream));
    *L = LensSystem{g.lens_elements, g.lens_bounds, d->n_lens_elements, d->n_exit_pupil_bounds, d->film_diagonal, (float)d->full_res[0], (float)d->full_res[1],
                    d->shutter_open, d->shutter_close, d->lens_simple_weighting ? 1u : 0u};
    return RSPT_OK;
}
// Argument validation of a render: fills the integrator / sampler flags and the sample range from the desc, touches no device state
int RenderRun::validate() {
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (!s || !d) return fail(RSPT_E_INVALID, "null scene or render desc");
    if ((shade_math = shade_math_mode()) < 0) return fail(RSPT_E_INVALID, "RSPT_SHADE_MATH=%s (exact or fast)", getenv("RSPT_SHADE_MATH"));
    if (int rc = validate_camera(d)) return rc;
    // ABI 26: the realistic camera is served where k_raygen_lens and the per-sample ray weight are: path and ao in the wavefront form (Sobol' / Halton).  The
    // schedules of volpath, directlighting and whitted consume k_raygen's output in their own ways and the pixel samplers' per-tile walk makes its own camera
    // rays (tile_serial.h): refused, so the caller keeps its CPU loop.
    realistic = d->camera_kind == RSPT_CAMERA_REALISTIC;
    if (realistic) {
        static const char* const names[] = {"path", "ao", "directlighting", "volpath", "whitted"};
        if (d->integrator != RSPT_INTEGRATOR_PATH && d->integrator != RSPT_INTEGRATOR_AO)
            return fail(RSPT_E_UNSUPPORTED, "the realistic camera under the %s integrator: it is served by path and ao only (their schedules carry the ray weight)", d->integrator < 5 ? names[d->integrator] : "?");
        if (d->sampler_kind != RSPT_SAMPLER_SOBOL && d->sampler_kind != RSPT_SAMPLER_HALTON)
            return fail(RSPT_E_UNSUPPORTED, "the realistic camera under the %s sampler: it is served with the sobol and halton samplers only (a pixel sampler's tile walk makes its own camera rays)",
                        d->sampler_kind == RSPT_SAMPLER_RANDOM ? "random" : d->sampler_kind == RSPT_SAMPLER_ZEROTWO ? "02sequence" : d->sampler_kind == RSPT_SAMPLER_STRATIFIED ? "stratified" :
                        d->sampler_kind == RSPT_SAMPLER_MAXMINDIST ? "maxmindist" : "unknown");
    }
    // Analytic spheres are served as surfaces (hit, shaded, textured, blocking light) by the path and AO integrators in their wavefront form
    // (Sobol' / Halton).  Everything else that holds a sphere is refused, so the caller keeps its CPU loop: sphere area lights (their
    // sample_with_ref_point / pdf_with_ref_point and power are not on the device), the directlighting / whitted / volpath forms and the pixel
    // samplers (their per-lane walks, trace_serial.h, have no sphere test), and a sphere scene whose records outgrow the four-box kernel.
    // ABI 27: disks and cylinders are served exactly where spheres are; their refusals name them (a scene without one keeps the sphere wording below)
    if (s->has_quadrics) {
        static const char* const names[] = {"path", "ao", "directlighting", "volpath", "whitted"};
        const char* iname = d->integrator < 5 ? names[d->integrator] : "?";
        const char* q = s->quadric_kinds;
        // In such a scene a shape's area light is served only while that shape's gate is on: an emissive disk or cylinder needs the quadric-light gate
        // (rspt_set_quadric_lights), an emissive sphere both gates.  With the quadric gate off every answer below is the one from before that gate existed.
        if (s->quadric_light_kinds) {
            const int ql = quadric_lights_mode();
            if (ql < 0) return fail(RSPT_E_INVALID, "RSPT_QUADRIC_LIGHTS=%s: 0 or 1", getenv("RSPT_QUADRIC_LIGHTS"));
            if (!ql) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive %s: %s are not served on the device yet (%s)", s->quadric_light_kinds, s->quadric_light_what, iname);
            quadric_lights = true;
        }
        if (s->has_sphere_light) {
            const int sl = sphere_lights_mode();   // the gate (rspt_set_sphere_lights)
            if (sl < 0) return fail(RSPT_E_INVALID, "RSPT_SPHERE_LIGHTS=%s: 0 or 1", getenv("RSPT_SPHERE_LIGHTS"));
            const int ql = quadric_lights ? 1 : quadric_lights_mode();
            if (!sl && ql == 1) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere next to a %s: a sphere area light there needs the sphere-light gate too (rspt_set_sphere_lights) (%s)", q, iname);
            if (!sl) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere next to a %s: sphere area lights are not served on the device yet (%s)", q, iname);
            if (ql < 0) return fail(RSPT_E_INVALID, "RSPT_QUADRIC_LIGHTS=%s: 0 or 1", getenv("RSPT_QUADRIC_LIGHTS"));
            if (!ql) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere next to a %s: sphere area lights are served in scenes without a disk or a cylinder only (%s)", q, iname);
            quadric_lights = true;
        }
        if (quadric_lights) {
            // Served by path under Sobol' / Halton (the quadric-light shade sets, launch_trace.h) and by ao, which reads no lights; everything else is refused by
            // name ("disk area light" / "cylinder area light"; "sphere area light" where only a sphere emits), so the caller keeps its CPU loop.
            const char* what = quadric_scene_lights_what(s);
            if (d->integrator != RSPT_INTEGRATOR_PATH && d->integrator != RSPT_INTEGRATOR_AO)
                return fail(RSPT_E_UNSUPPORTED, "scene with %s under the %s integrator: these lights are served by path (and ao, which reads no lights) only", what, iname);
            if (d->sampler_kind != RSPT_SAMPLER_SOBOL && d->sampler_kind != RSPT_SAMPLER_HALTON)
                return fail(RSPT_E_UNSUPPORTED, "scene with %s under the %s sampler: these lights are served with the sobol and halton samplers only", what,
                            d->sampler_kind == RSPT_SAMPLER_RANDOM ? "random" : d->sampler_kind == RSPT_SAMPLER_ZEROTWO ? "02sequence" : d->sampler_kind == RSPT_SAMPLER_STRATIFIED ? "stratified" :
                            d->sampler_kind == RSPT_SAMPLER_MAXMINDIST ? "maxmindist" : "unknown");
            if (!s->w4_ok) return fail(RSPT_E_UNSUPPORTED, "scene with %s and more four-box records than a reference holds", what);
            if (env_size("RSPT_COUNTERS", 0) != 0) return fail(RSPT_E_UNSUPPORTED, "RSPT_COUNTERS on a scene with %s: the quadric traversal keeps no node counters", what);
            if (s->has_maplights) return fail(RSPT_E_UNSUPPORTED, "scene with a %s light next to %s: that pair has no shade instantiation", s->maplight_kinds, what);
        }
        if (d->integrator != RSPT_INTEGRATOR_PATH && d->integrator != RSPT_INTEGRATOR_AO)
            return fail(RSPT_E_UNSUPPORTED, "scene with a %s under the %s integrator: these shapes are served by path and ao only", q, iname);
        if (d->sampler_kind != RSPT_SAMPLER_SOBOL && d->sampler_kind != RSPT_SAMPLER_HALTON)
            return fail(RSPT_E_UNSUPPORTED, "scene with a %s under the %s sampler: these shapes are served with the sobol and halton samplers only", q,
                        d->sampler_kind == RSPT_SAMPLER_RANDOM ? "random" : d->sampler_kind == RSPT_SAMPLER_ZEROTWO ? "02sequence" : d->sampler_kind == RSPT_SAMPLER_STRATIFIED ? "stratified" :
                        d->sampler_kind == RSPT_SAMPLER_MAXMINDIST ? "maxmindist" : "unknown");
        if (!s->w4_ok) return fail(RSPT_E_UNSUPPORTED, "%s scene with more four-box records than a reference holds", q);
        if (env_size("RSPT_COUNTERS", 0) != 0) return fail(RSPT_E_UNSUPPORTED, "RSPT_COUNTERS on a scene with a %s: the quadric traversal keeps no node counters", q);
        if (s->has_maplights) return fail(RSPT_E_UNSUPPORTED, "scene with a %s light next to a %s: that pair has no shade instantiation yet", s->maplight_kinds, q);
    } else
    if (s->has_spheres) {
        static const char* const names[] = {"path", "ao", "directlighting", "volpath", "whitted"};
        const char* iname = d->integrator < 5 ? names[d->integrator] : "?";
        if (s->has_sphere_light) {
            // The gate (rspt_set_sphere_lights).  Off: today's answer.  On: served by path under Sobol' / Halton (the sphere-light shade sets, launch_trace.h) and by ao,
            // which reads no lights; everything else is refused by name, so the caller keeps its CPU loop.
            const int sl = sphere_lights_mode();
            if (sl < 0) return fail(RSPT_E_INVALID, "RSPT_SPHERE_LIGHTS=%s: 0 or 1", getenv("RSPT_SPHERE_LIGHTS"));
            if (!sl) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere: sphere area lights are not served on the device yet (%s)", iname);
            if (d->integrator != RSPT_INTEGRATOR_PATH && d->integrator != RSPT_INTEGRATOR_AO)
                return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere under the %s integrator: sphere area lights are served by path (and ao, which reads no lights) only", iname);
            if (d->sampler_kind != RSPT_SAMPLER_SOBOL && d->sampler_kind != RSPT_SAMPLER_HALTON)
                return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere under the %s sampler: sphere area lights are served with the sobol and halton samplers only",
                            d->sampler_kind == RSPT_SAMPLER_RANDOM ? "random" : d->sampler_kind == RSPT_SAMPLER_ZEROTWO ? "02sequence" : d->sampler_kind == RSPT_SAMPLER_STRATIFIED ? "stratified" :
                            d->sampler_kind == RSPT_SAMPLER_MAXMINDIST ? "maxmindist" : "unknown");
            if (!s->w4_ok) return fail(RSPT_E_UNSUPPORTED, "scene with a sphere area light and more four-box records than a reference holds");
            if (env_size("RSPT_COUNTERS", 0) != 0) return fail(RSPT_E_UNSUPPORTED, "RSPT_COUNTERS on a scene with a sphere area light: the sphere traversal keeps no node counters");
            if (s->has_maplights) return fail(RSPT_E_UNSUPPORTED, "scene with a %s light next to a sphere area light: that pair has no shade instantiation", s->maplight_kinds);
            sphere_lights = true;
        }
        if (d->integrator != RSPT_INTEGRATOR_PATH && d->integrator != RSPT_INTEGRATOR_AO)
            return fail(RSPT_E_UNSUPPORTED, "scene with spheres under the %s integrator: spheres are served by path and ao only", iname);
        if (d->sampler_kind != RSPT_SAMPLER_SOBOL && d->sampler_kind != RSPT_SAMPLER_HALTON)
            return fail(RSPT_E_UNSUPPORTED, "scene with spheres under the %s sampler: spheres are served with the sobol and halton samplers only",
                        d->sampler_kind == RSPT_SAMPLER_RANDOM ? "random" : d->sampler_kind == RSPT_SAMPLER_ZEROTWO ? "02sequence" : d->sampler_kind == RSPT_SAMPLER_STRATIFIED ? "stratified" :
                        d->sampler_kind == RSPT_SAMPLER_MAXMINDIST ? "maxmindist" : "unknown");
        if (!s->w4_ok) return fail(RSPT_E_UNSUPPORTED, "sphere scene with more four-box records than a reference holds");
        if (env_size("RSPT_COUNTERS", 0) != 0) return fail(RSPT_E_UNSUPPORTED, "RSPT_COUNTERS on a scene with spheres: the sphere traversal keeps no node counters");
    }
    // ABI 24: projection and goniometric lights are served where their two arms of light_sample_li / light_is_delta are compiled: the path integrator's wavefront
    // form under Sobol' / Halton (the map-light shade instantiations, launch_trace.h) and ao, which reads no lights.  The per-lane and per-tile walks of the other
    // integrators and of the pixel samplers keep their code, so everything else is refused and the caller keeps its CPU loop.
    if (s->has_maplights) {
        static const char* const names[] = {"path", "ao", "directlighting", "volpath", "whitted"};
        const char* iname = d->integrator < 5 ? names[d->integrator] : "?";
        if (d->integrator != RSPT_INTEGRATOR_PATH && d->integrator != RSPT_INTEGRATOR_AO)
            return fail(RSPT_E_UNSUPPORTED, "scene with a %s light under the %s integrator: these lights are served by path (and ao, which reads none) only", s->maplight_kinds, iname);
        if (d->sampler_kind != RSPT_SAMPLER_SOBOL && d->sampler_kind != RSPT_SAMPLER_HALTON)
            return fail(RSPT_E_UNSUPPORTED, "scene with a %s light under the %s sampler: these lights are served with the sobol and halton samplers only", s->maplight_kinds,
                        d->sampler_kind == RSPT_SAMPLER_RANDOM ? "random" : d->sampler_kind == RSPT_SAMPLER_ZEROTWO ? "02sequence" : d->sampler_kind == RSPT_SAMPLER_STRATIFIED ? "stratified" :
                        d->sampler_kind == RSPT_SAMPLER_MAXMINDIST ? "maxmindist" : "unknown");
        if (s->has_spheres) return fail(RSPT_E_UNSUPPORTED, "scene with a %s light next to analytic spheres: that pair has no shade instantiation yet", s->maplight_kinds);
    }
    // WhittedIntegrator::li runs on directlighting's machinery (direct.h / dl_serial.h, their WH forms) as UniformSampleAll with one estimate per light and
    // no sample arrays; max_depth 0 recurses no more than 1 does (whitted.rs:103: depth + 1 < max_depth)
    whitted = d->integrator == RSPT_INTEGRATOR_WHITTED;
    if (whitted) {
        wd = *d;
        wd.direct_strategy = RSPT_DIRECT_SAMPLE_ALL;
        wd.n_light_samples = nullptr;
        if (wd.max_depth == 0) wd.max_depth = 1;
        d = &wd;
    }
    dl_name = whitted ? "whitted" : "directlighting";
    multi_lobes = d->integrator != RSPT_INTEGRATOR_DIRECT && !whitted;  // allow_multiple_lobes: false in DirectLightingIntegrator::li and WhittedIntegrator::li (directlighting.rs:86, whitted.rs:63)
    halton = d->sampler_kind == RSPT_SAMPLER_HALTON;
    sobol = d->sampler_kind == RSPT_SAMPLER_SOBOL;
    pixel_sampler = d->sampler_kind >= RSPT_SAMPLER_RANDOM && d->sampler_kind <= RSPT_SAMPLER_MAXMINDIST;  // one serial chain per tile: tile_serial.h
    if (!sobol && !halton && !pixel_sampler) return fail(RSPT_E_UNSUPPORTED, "sampler kind %u", d->sampler_kind);
    if (d->spp <= 0 || d->spp > (1ll << 30) || (sobol && (d->spp & (d->spp - 1)) != 0)) return fail(RSPT_E_INVALID, "spp must be in [1, 2^30] (a power of two for sobol)");
    if (d->tile_size == 0 || d->tile_size > 4096) return fail(RSPT_E_INVALID, "bad tile_size");
    if (sobol && (!d->tables.sobol32 || !d->tables.vdc || !d->tables.vdc_inv)) return fail(RSPT_E_INVALID, "null sobol tables");
    if (pixel_sampler) {
        if (d->integrator == RSPT_INTEGRATOR_DIRECT && d->direct_strategy == RSPT_DIRECT_SAMPLE_ALL && (d->sampler_kind == RSPT_SAMPLER_ZEROTWO || d->sampler_kind == RSPT_SAMPLER_MAXMINDIST))
            for (uint32_t i = 0; s && d->n_light_samples && i < s->dev.n_lights; i++)
                if (d->n_light_samples[i] < 1 || (d->n_light_samples[i] & (d->n_light_samples[i] - 1)) != 0)
                    return fail(RSPT_E_INVALID, "directlighting: n_light_samples[%u] must be a power of two with the 02sequence / maxmindist samplers (preprocess passes it through round_count, directlighting.rs:58-60)", i);
        if (d->integrator == RSPT_INTEGRATOR_AO && (d->sampler_kind == RSPT_SAMPLER_ZEROTWO || d->sampler_kind == RSPT_SAMPLER_MAXMINDIST) && (d->ao_n_samples & (d->ao_n_samples - 1)) != 0)
            return fail(RSPT_E_INVALID, "ao: nsamples must be a power of two with the 02sequence / maxmindist samplers (request_2d_array asserts round_count(n) == n, zerotwosequence.rs:187-193)");
        if (d->tile_size > 255) return fail(RSPT_E_UNSUPPORTED, "tile_size > 255 with a pixel sampler");
        if (d->spp > 65536 || d->pixel_dimensions > 64) return fail(RSPT_E_UNSUPPORTED, "pixel sampler: spp > 65536 or more than 64 sampled dimensions");
        if (d->sampler_kind == RSPT_SAMPLER_STRATIFIED && (d->strat_x == 0 || d->strat_y == 0 || (int64_t)d->strat_x * d->strat_y != d->spp))
            return fail(RSPT_E_INVALID, "stratified sampler: spp must equal strat_x * strat_y");
        if (d->sampler_kind == RSPT_SAMPLER_MAXMINDIST && (!d->maxmin_c_pixel || (d->spp & (d->spp - 1)) != 0)) return fail(RSPT_E_INVALID, "maxmindist sampler: spp must be a power of two and maxmin_c_pixel given");
    }
    if (halton && !d->tables.halton_perms) return fail(RSPT_E_INVALID, "null halton permutation table");
    if (!(d->filter_radius[0] > 0.0f) || !(d->filter_radius[1] > 0.0f)) return fail(RSPT_E_INVALID, "bad filter radius");
    if (d->max_depth > 200) return fail(RSPT_E_UNSUPPORTED, "max_depth > 200");
    if (d->integrator != RSPT_INTEGRATOR_PATH && d->integrator != RSPT_INTEGRATOR_AO && d->integrator != RSPT_INTEGRATOR_DIRECT && d->integrator != RSPT_INTEGRATOR_VOLPATH && !whitted)
        return fail(RSPT_E_UNSUPPORTED, "integrator %u (path, ao, directlighting, volpath and whitted only)", d->integrator);
    direct = d->integrator == RSPT_INTEGRATOR_DIRECT || whitted;   // (the directlighting forms; `whitted` picks their WH instantiations)
    volpath = d->integrator == RSPT_INTEGRATOR_VOLPATH;
    // moving instances under the pixel samplers and in the per-lane directlighting: round 6 (k_tile_serial modes 5 - 8, k_lane_dl<.., ANIM>); dynamic materials next to them under a
    // pixel sampler are the one combination left without an instantiation
    if (s->has_animated && pixel_sampler && s->mat_set[multi_lobes ? 0 : 1].dynamic)
        return fail(RSPT_E_UNSUPPORTED, "a scene with a moving object instance AND a dynamic material (a lobe list that depends on a texture value) under a pixel sampler");
    if (direct) {
        if (d->max_depth < 1 || d->max_depth > (uint32_t)RSPT_DL_SERIAL_DEPTH)
            return fail(RSPT_E_UNSUPPORTED, "%s: max_depth must be in [%d, %d] (the explicit recursion stack of the per-lane form, dl_serial.h)", dl_name, whitted ? 0 : 1, RSPT_DL_SERIAL_DEPTH);
        if (whitted && s->dev.n_lights > (1u << 16)) return fail(RSPT_E_UNSUPPORTED, "whitted: more than 65536 lights (one estimate per light and node in one round, direct.h)");
        if (d->direct_strategy > RSPT_DIRECT_SAMPLE_ONE) return fail(RSPT_E_INVALID, "bad direct_strategy");
        for (uint32_t i = 0; s && d->n_light_samples && i < s->dev.n_lights; i++)
            if (d->n_light_samples[i] < 1 || d->n_light_samples[i] > 4096) return fail(RSPT_E_INVALID, "n_light_samples[%u] out of range", i);
    }
    if (d->integrator == RSPT_INTEGRATOR_AO && (d->ao_n_samples == 0 || d->ao_n_samples > 4096)) return fail(RSPT_E_INVALID, "ao_n_samples must be in [1, 4096]");
    // checkpoint / resume: the pixel samples [smp_begin, smp_end) of every pixel
    smp_begin = d->sample_begin; smp_end = d->sample_count ? d->sample_begin + d->sample_count : (uint64_t)d->spp;
    if (smp_begin >= smp_end || smp_end > (uint64_t)d->spp) return fail(RSPT_E_INVALID, "sample range [%llu, %llu) outside [0, spp)", (unsigned long long)smp_begin, (unsigned long long)smp_end);
    if (pixel_sampler && (smp_begin != 0 || smp_end != (uint64_t)d->spp)) return fail(RSPT_E_UNSUPPORTED, "a pixel sampler renders all samples of a tile in one chain: partial sample ranges are not possible");
    sb = d->sample_bounds;
    cp = d->crop_px;
    if (sb[2] <= sb[0] || sb[3] <= sb[1] || cp[2] <= cp[0] || cp[3] <= cp[1]) return fail(RSPT_E_INVALID, "empty sample or crop bounds");
    if (sb[0] < -32768 || sb[1] < -32768 || sb[2] > 32767 || sb[3] > 32767) return fail(RSPT_E_UNSUPPORTED, "sample bounds outside the 16-bit pixel range");
    shard_count = d->shard_count ? d->shard_count : 1; chunk = d->tile_chunk ? d->tile_chunk : 1;
    if (d->shard_index >= shard_count) return fail(RSPT_E_INVALID, "shard_index >= shard_count");
    // Sobol' needs 5 + 8 dims per bounce < 1024 (sobol.rs:119-124)
    if (5ull + (volpath ? 10ull : 8ull) * (d->max_depth + 2ull) >= 1024ull) return fail(RSPT_E_UNSUPPORTED, "max_depth exceeds the 1024 Sobol' dimensions");
    return RSPT_OK;
}
int RenderRun::constants() {
    int rc;
    // ---- render constants ----
    memcpy(rd.raster_to_camera, d->raster_to_camera, sizeof rd.raster_to_camera);
    memcpy(rd.camera_to_world, d->camera_to_world, sizeof rd.camera_to_world);
    rd.lens_radius = d->lens_radius; rd.focal_distance = d->focal_distance;
    rd.camera_kind = d->camera_kind; rd.full_res[0] = d->full_res[0]; rd.full_res[1] = d->full_res[1];
    rd.cam_anim = nullptr;
    if (d->camera_animated) {   // AnimatedTransform::new (camera_anim.h); equal key matrices = a camera that does not move
        CamAnim ca;
        if (camanim::camera_keys(d->camera_to_world, d->camera_time[0], d->camera_to_world_end, d->camera_time[1], &ca)) {
            if (!g.cam_anim && (rc = dev_alloc(&g.cam_anim, 1))) return rc;
            HIP_TRY(hipMemcpy(g.cam_anim, &ca, sizeof ca, hipMemcpyHostToDevice));
            rd.cam_anim = g.cam_anim;
        }
    }
    rd.shutter_open = d->shutter_open; rd.shutter_close = d->shutter_close;
    if (realistic && (rc = upload_lens(d, &lens))) return rc;
    memcpy(rd.sample_bounds, sb, sizeof rd.sample_bounds);
    memcpy(rd.crop_px, cp, sizeof rd.crop_px);
    rd.resolution = round_up_pow2_32(std::max(sb[2] - sb[0], sb[3] - sb[1]));  // sobol.rs:46-47
    rd.log2_res = 31 - __builtin_clz((uint32_t)rd.resolution);
    rd.spp = d->spp; rd.max_depth = d->max_depth; rd.rr_threshold = d->rr_threshold;
    rd.filter_radius[0] = d->filter_radius[0]; rd.filter_radius[1] = d->filter_radius[1];
    rd.max_sample_luminance = d->max_sample_luminance;
    rd.tile_size = d->tile_size;
    if (!g.sobol32) {
        if ((rc = dev_alloc(&g.sobol32, 1024 * 52)) || (rc = dev_alloc(&g.vdc, 25 * 52)) || (rc = dev_alloc(&g.vdc_inv, 26 * 52)) || (rc = dev_alloc(&g.filter_table, 256))) return rc;
    }
    if (sobol) {
        HIP_TRY(hipMemcpyAsync(g.sobol32, d->tables.sobol32, 1024 * 52 * 4, hipMemcpyHostToDevice, g.stream));
        HIP_TRY(hipMemcpyAsync(g.vdc, d->tables.vdc, 25 * 52 * 8, hipMemcpyHostToDevice, g.stream));
        HIP_TRY(hipMemcpyAsync(g.vdc_inv, d->tables.vdc_inv, 26 * 52 * 8, hipMemcpyHostToDevice, g.stream));
    }
    HIP_TRY(hipMemcpyAsync(g.filter_table, d->filter_table, 256 * 4, hipMemcpyHostToDevice, g.stream));
    rd.sobol32 = g.sobol32; rd.vdc = g.vdc; rd.vdc_inv = g.vdc_inv; rd.filter_table = g.filter_table;
    rd.sampler_kind = d->sampler_kind;
    rd.sample_at_pixel_center = d->sample_at_pixel_center;
    vol_dim_limit = 1024u;  // NUM_SOBOL_DIMENSIONS (sobol.rs:119-124) or the Halton permutation table the caller brought
    if (halton) {  // HaltonSampler::new (halton.rs:80-131)
        if (!g.primes) {  // PRIMES / PRIME_SUMS (lowdiscrepancy.rs:31-760)
            std::vector<uint32_t> primes, sums;
            for (uint32_t v = 2; primes.size() < 1000; v++) {
                bool is_p = true;
                for (uint32_t q = 2; q * q <= v; q++) if (v % q == 0) { is_p = false; break; }
                if (is_p) primes.push_back(v);
            }
            uint32_t acc = 0;
            for (uint32_t p : primes) { sums.push_back(acc); acc += p; }
            g.host_primes = primes; g.host_prime_sums = sums;
            if ((rc = dev_alloc(&g.primes, 1000)) || (rc = dev_alloc(&g.prime_sums, 1000))) return rc;
            HIP_TRY(hipMemcpy(g.primes, primes.data(), 4000, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(g.prime_sums, sums.data(), 4000, hipMemcpyHostToDevice));
        }
        uint32_t max_dim = 5u + 8u * (d->max_depth + 2u);  // last dimension a path can consume, with slack
        if (volpath) max_dim = std::min(990u, 5u + 10u * (d->max_depth + 2u) + 64u);  // 10 per counted bounce, 2 per uncounted pass through a medium boundary (slack for 32; vol.h cuts a path that needs more)
        if (direct) {  // every dimension the caller's table covers: k_dl_assign reports a camera sample whose stream really ends beyond it
            max_dim = 0;
            while (max_dim + 1u < 1000u && (uint64_t)g.host_prime_sums[max_dim + 1u] + g.host_primes[max_dim + 1u] <= d->tables.n_halton_perms) max_dim++;
        }
        if (max_dim >= 1000u) return fail(RSPT_E_UNSUPPORTED, "max_depth exceeds the 1000 Halton dimensions");
        const uint64_t need = (uint64_t)g.host_prime_sums[max_dim] + g.host_primes[max_dim];
        if (d->tables.n_halton_perms < need) return fail(RSPT_E_INVALID, "halton permutation table has %llu entries, %llu needed for max_depth %u",
                                                         (unsigned long long)d->tables.n_halton_perms, (unsigned long long)need, d->max_depth);
        if ((rc = ensure_array(&g.halton_perms, &g.n_halton_perms, need))) return rc;
        HIP_TRY(hipMemcpyAsync(g.halton_perms, d->tables.halton_perms, need * sizeof(uint16_t), hipMemcpyHostToDevice, g.stream));
        rd.halton_perms = g.halton_perms; rd.primes = g.primes; rd.prime_sums = g.prime_sums;
        vol_dim_limit = max_dim;
        const int32_t res[2] = {sb[2] - sb[0], sb[3] - sb[1]};
        for (int i = 0; i < 2; i++) {
            int32_t base = i == 0 ? 2 : 3, scale = 1, exp = 0;
            while (scale < std::min(res[i], 128)) { scale *= base; exp += 1; }
            rd.base_scales[i] = scale; rd.base_exponents[i] = exp;
        }
        rd.sample_stride = (uint64_t)rd.base_scales[0] * (uint64_t)rd.base_scales[1];
        auto mult_inv = [](int64_t a, int64_t n) {  // multiplicative_inverse via extended_gcd (halton.rs:32-52)
            int64_t x0 = 1, x1 = 0, r0 = a, r1 = n;
            while (r1 != 0) {
                int64_t q = r0 / r1, t = r0 - q * r1;
                r0 = r1; r1 = t;
                t = x0 - q * x1; x0 = x1; x1 = t;
            }
            int64_t m = x0 % n;
            return (uint64_t)(m < 0 ? m + n : m);
        };
        rd.mult_inverse[0] = mult_inv(rd.base_scales[1], rd.base_scales[0]);
        rd.mult_inverse[1] = mult_inv(rd.base_scales[0], rd.base_scales[1]);
    }

    if ((rc = get_light_dist(s, d->light_strategy, &ld, &ld_lazy))) return rc;
    // (k_ld_mark finds a hit's voxel from its barycentrics: a sphere scene takes the eager table or nothing)
    if (ld_lazy && s->has_quadrics) return fail(RSPT_E_UNSUPPORTED, "scene with a %s whose spatial light table needs on-demand voxels (more than RSPT_LIGHT_TABLE_EAGER_BYTES)", s->quadric_kinds);
    if (ld_lazy && s->has_spheres) return fail(RSPT_E_UNSUPPORTED, "scene with spheres whose spatial light table needs on-demand voxels (more than RSPT_LIGHT_TABLE_EAGER_BYTES)");
    if (volpath && s->dev.n_grid_media && !pixel_sampler)
        return fail(RSPT_E_UNSUPPORTED, "volpath with a grid-density medium under the Sobol' / Halton sampler: every tracking step draws sampler dimensions (the reference panics past "
                                        "dimension 1024 / 1000 within a bounce or two); render it with a pixel sampler (random / 02sequence / stratified / maxmindist)");
    // on-demand voxels under volpath and the pixel samplers: their kernels meet the lookup points only while they run, so they claim missing
    // voxels themselves (dev_scene.h light_row_try) and the step runs again once the claimed rows are built (lightdistrib.rs:276-384 builds on
    // first touch too; a row is a pure function of (voxel, lights), Q18, so when it is built cannot show)
    if (ld_lazy && (volpath || pixel_sampler)) { ld.lazy = reinterpret_cast<LightLazyWords*>(ld_lazy->lazy); ld.new_list = ld_lazy->new_list; }
    static_assert(sizeof(LightLazyWords) == sizeof(LightLazy), "LightLazyWords mirrors LightLazy");
    return RSPT_OK;
}
int RenderRun::shard_pixels() {
    int rc;
    // ---- this shard's pixels: Morton-ordered tiles (blockqueue/mod.rs:23-52), row-major inside a tile ----
    ts = (int32_t)d->tile_size;
    const int32_t ext_x = sb[2] - sb[0], ext_y = sb[3] - sb[1];
    ntx = (ext_x + ts - 1) / ts; const int32_t nty = (ext_y + ts - 1) / ts;
    std::vector<std::pair<uint32_t, uint32_t>> blocks((size_t)ntx * nty);
    for (int32_t i = 0; i < ntx * nty; i++) blocks[i] = {(uint32_t)(i % ntx), (uint32_t)(i / ntx)};
    std::stable_sort(blocks.begin(), blocks.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return morton2(a.first, a.second) < morton2(b.first, b.second); });
    n_blocks = blocks.size();
    for (size_t i = 0; i < blocks.size(); i++)   // (every shard_count-th chunk of the Morton order)
        if ((i / chunk) % shard_count == d->shard_index) shard_tiles.push_back(blocks[i]);
    pix.reserve((size_t)ext_x * ext_y / shard_count + 1024);
    for (const auto& b : shard_tiles) {
        int32_t x0 = sb[0] + (int32_t)b.first * ts, x1 = std::min(x0 + ts, sb[2]);
        int32_t y0 = sb[1] + (int32_t)b.second * ts, y1 = std::min(y0 + ts, sb[3]);
        for (int32_t y = y0; y < y1; y++)
            for (int32_t x = x0; x < x1; x++) pix.push_back(((uint32_t)(uint16_t)(int16_t)y << 16) | (uint32_t)(uint16_t)(int16_t)x);
    }
    n_pix = pix.size();
    if ((rc = ensure_array(&g.pix_list, &g.pix_cap, n_pix))) return rc;
    if (n_pix) HIP_TRY(hipMemcpyAsync(g.pix_list, pix.data(), n_pix * 4, hipMemcpyHostToDevice, g.stream));
    return RSPT_OK;
}
int RenderRun::film_buffers(const float* li_host) {
    int rc;
    // ---- film ----
    film_px = (size_t)(cp[2] - cp[0]) * (size_t)(cp[3] - cp[1]);
    if (g.film_px < film_px) {
        for (float4** p : {&g.film_own, &g.film_splat, &g.film_out}) { if (*p) (void)hipFree(*p); *p = nullptr; }
        g.film_px = 0;
        if ((rc = dev_alloc(&g.film_own, film_px)) || (rc = dev_alloc(&g.film_splat, film_px)) || (rc = dev_alloc(&g.film_out, film_px))) return rc;
        g.film_px = film_px;
    }
    HIP_TRY(hipMemsetAsync(g.film_own, 0, film_px * sizeof(float4), g.stream));
    HIP_TRY(hipMemsetAsync(g.film_splat, 0, film_px * sizeof(float4), g.stream));
    // the film stage: k_film, or for filters wider than a pixel the gather form (kernels.h k_film_gather; RSPT_FILM_GATHER=0: the atomic form)
    film_k = (int)std::floor(std::max(d->filter_radius[0], d->filter_radius[1]) + 0.5f);
    film_gather = (d->filter_radius[0] > 0.5f || d->filter_radius[1] > 0.5f) && film_k <= 8 && env_size("RSPT_FILM_GATHER", 1) != 0;
    sb_px = (size_t)(sb[2] - sb[0]) * (size_t)(sb[3] - sb[1]);
    if (film_gather && (rc = ensure_array(&g.pix_index, &g.pix_index_cap, sb_px))) return rc;
    if (li_host) {
        HIP_TRY(hipMalloc((void**)&li_dev, film_px * (size_t)d->spp * 3 * sizeof(float)));
        temps.p.push_back(li_dev);   // (freed with the run, also on the early error returns)
        HIP_TRY(hipMemsetAsync(li_dev, 0, film_px * (size_t)d->spp * 3 * sizeof(float), g.stream));
    }
    return RSPT_OK;
}
int RenderRun::film_index(const uint32_t* list, uint32_t n) {   // (the list a batch indexes: the render's, or one pass of the pixel samplers)
    if (!film_gather) return RSPT_OK;
    HIP_TRY(hipMemsetAsync(g.pix_index, 0xff, sb_px * sizeof(uint32_t), g.stream));
    if (n) hipLaunchKernelGGL(k_pix_index, dim3((n + 255) / 256), dim3(256), 0, g.stream, list, n, sb[0], sb[1], sb[2] - sb[0], g.pix_index);
    return RSPT_OK;
}
void RenderRun::film_stage(const RenderDev& rd_, const Batch& bt, const PathBuf& fpb, const uint32_t* list) {
    if (!film_gather) {
        hipLaunchKernelGGL(k_film, dim3((bt.n_pix + 255) / 256), dim3(256), 0, g.stream, rd_, bt, fpb, list, g.film_own, (float*)g.film_splat, li_dev, g.totals + 5);
        return;
    }
    const size_t s2 = (size_t)(RSPT_FG_T + 2 * film_k) * (RSPT_FG_T + 2 * film_k);
    const size_t fit = (60000 - s2 * 4 - 1024) / (s2 * 24);   // sample rows of (chunk + 1) x 24 bytes per source pixel in < 64 KB of LDS
    const uint32_t chunk = (uint32_t)std::min<size_t>(std::max<size_t>(fit, 2) - 1, 8);
    const size_t lds = s2 * (chunk + 1) * 24 + s2 * 4 + 1024;
    hipLaunchKernelGGL(k_film_gather, dim3((uint32_t)((sb[2] - sb[0] + RSPT_FG_T - 1) / RSPT_FG_T), (uint32_t)((sb[3] - sb[1] + RSPT_FG_T - 1) / RSPT_FG_T)), dim3(256), lds, g.stream,
                       rd_, bt, fpb, g.pix_index, film_k, chunk, g.film_own, li_dev, g.totals + 5);
}
int RenderRun::size_batches() {
    int rc;
    // ---- batches ----
    // paths per wavefront batch: ~280 B of state each, so 2^29 paths = 150 GB of the 288 GB HBM.  Large batches keep the persistent
    // trace kernel's queues long and its launches few (every launch ends in a tail of a few long rays): measured with round 1's
    // kernels, 2^25 / 2^26 / 2^27 / 2^28 paths per batch = 367 / 386 / 398 / 405 Msamples/s on C2 and 1243 / 1400 / 1472 / 1525 on
    // the C3 stand-in; with round 4's, 2^28 -> 2^29 on the C3 stand-in: 1929 -> 1966 (same box; C2's frame is 2^28 paths, one batch
    // either way).  Halving the number of launch tails bought 1.9 %: what is left of them is what a second pipeline of half batches
    // on other streams could still fill — less than that again, which is why shade / trace overlap across batches was not built
    // (DESIGN.md section 10).  When the device cannot give that much (other tenants), the batch is halved until it fits.
    cap = env_size("RSPT_BATCH", (size_t)1 << 29);
    cap = std::min<size_t>(std::max<size_t>(cap, 1024), (size_t)1 << 30);
    counters = env_size("RSPT_COUNTERS", 0) != 0;
    // AOIntegrator: every camera sample carries ao_n_samples shadow rays through the same ray / occlusion arrays
    ao = d->integrator == RSPT_INTEGRATOR_AO;
    ao_n = ao ? d->ao_n_samples : 1u;
    if (ao) cap = std::max<size_t>(cap / ao_n, 1024);
    // directlighting under Sobol' / Halton: the wavefront form (direct.h) unless the render needs what only the per-lane form has
    // (lane_serial.h): textured materials, more than 8 recursion levels; RSPT_DL_FORM=lane forces it (A/B, tests)
    const char* dl_form_env = getenv("RSPT_DL_FORM");
    // levels of the specular tree that can hold nodes (direct.h DlBuf::levels): a scene without specular lobes has the root only
    const bool dl_specular = s->has_dynamic || (s->shade_features & (RSPT_SF_LOBE(RSPT_BXDF_SPECULAR_R) | RSPT_SF_LOBE(RSPT_BXDF_SPECULAR_T) | RSPT_SF_LOBE(RSPT_BXDF_FRESNEL_SPEC))) != 0;
    // round 6: textured materials WITHOUT specular lobes stay in the wavefront form (every node is a camera hit: k_dl_texture); with specular lobes the children's rays carry
    // reflected / refracted differentials, which only the per-lane form tracks.  RSPT_DL_TEX_WAVEFRONT=0: textures always per lane, as before.  (The estimate kernel of the
    // one-round form is the one that reads the texture results: RSPT_DL_ROUNDS=1 or more than 2^16 estimates per node also send a textured scene to the per-lane form.)
    // estimates per node under SAMPLE_ALL; up to 2^16 of them fit one round (whitted's estimates exist in the one-round form only)
    const bool dl_all = d->direct_strategy == RSPT_DIRECT_SAMPLE_ALL && s->dev.n_lights;
    uint64_t dl_sum = dl_all ? 0 : 1;
    for (uint32_t j = 0; dl_all && j < s->dev.n_lights; j++) dl_sum += d->n_light_samples ? (uint64_t)std::max<int32_t>(d->n_light_samples[j], 0) : 1u;
    const bool dl_rounds_one = (whitted || env_size("RSPT_DL_ROUNDS", 0) == 0) && dl_sum <= (1u << 16);
    const bool dl_tex_wave = s->has_textures && !dl_specular && dl_rounds_one && env_size("RSPT_DL_TEX_WAVEFRONT", 1) != 0;
    dl_lane = direct && !pixel_sampler && ((s->has_textures && !dl_tex_wave) || d->max_depth > 8 || (dl_form_env && !strcmp(dl_form_env, "lane")));
    dl_levels = (dl_specular || env_size("RSPT_DL_FULL_TREE", 0) != 0) ? (uint32_t)d->max_depth : std::min<uint32_t>((uint32_t)d->max_depth, 1u);
    dl_H = (direct && !pixel_sampler && !dl_lane) ? (1u << dl_levels) : 1u;   // node slots per camera sample (direct.h; in the per-lane forms a lane walks the tree itself)
    // all light estimates of a node in one round (direct.h k_dl_nee_all): R = sum_j n_j virtual slots per node slot in the ray / result arrays; RSPT_DL_ROUNDS=1 = one
    // round per estimate as before (R = 1 for the sizing)
    // (R used to be CLAMPED to 2^20 while the kernels iterate over the unclamped sum — virtual slots would alias.  A sum above 2^16 — hundreds of lights at thousands
    //  of samples each — takes the round-per-estimate form instead, whose slots do not depend on it; n_slots * R then stays far below the RSPT_Q_MIS bit: the batch is <= 2^28 / R)
    dl_one_round = direct && !pixel_sampler && !dl_lane && dl_rounds_one;
    dl_R = dl_one_round ? (uint32_t)std::max<uint64_t>(dl_sum, 1u) : 1u;
    if (direct) cap = std::max<size_t>(std::min<size_t>(cap, (size_t)1 << (dl_lane ? (s->has_dynamic ? 20 : 22) : (dl_R > 1 ? 28 : 26))) / dl_H / dl_R, 1024);   // (per-lane form: texture rows and lobe records per recursion level)
    if (pixel_sampler) cap = std::max<size_t>(n_blocks, 1024);   // one path slot per tile (tile_serial.h); the samples' results have their own arrays
    // round 6: the path integrator's MOVING path state (kernels.h PathBuf::move) — wherever the scene's shade instantiation has a MOVE form; not with moving instances
    // (their ray times are kept by original slot) and not under the pixel samplers / the other integrators, which keep slots for life.  RSPT_MOVE=0: slots, as before.
    // the fast-math builds (rspt_set_shade_math): the path integrator's wavefront form under Sobol' / Halton only, and only the sets that have them; every other render
    // of a fast-mode process runs the exact kernels under the plain name
    const bool want_fast = shade_math == RSPT_SHADE_MATH_FAST && d->integrator == RSPT_INTEGRATOR_PATH && !pixel_sampler;
    shade_k = shade_kernel_for(s->shade_features | (halton ? (uint32_t)SF_HALTON : (uint32_t)SF_SOBOL), &shade_name, &shade_move_k, want_fast && !sphere_lights && !quadric_lights, &shade_fast, sphere_lights, quadric_lights);
    if (shade_k && shade_fast) { snprintf(shade_name_fast, sizeof shade_name_fast, "%s-fast", shade_name); shade_name = shade_name_fast; }
    if (!shade_k) return fail(RSPT_E_UNSUPPORTED, s->has_maplights ? "RSPT_SHADE_VARIANT names no instantiation with the projection / goniometric arms (generic-maplight, all-maplight)"
                                                                  : quadric_lights ? "RSPT_SHADE_VARIANT names no instantiation with the disk / cylinder area light arms (generic-quadriclight, dynamic-quadriclight)"
                                                                  : s->has_quadrics ? "RSPT_SHADE_VARIANT names no instantiation with the disk / cylinder arm (generic-quadric, dynamic-quadric)"
                                                                  : sphere_lights ? "RSPT_SHADE_VARIANT names no instantiation with the sphere area light arms (generic-spherelight, dynamic-spherelight)"
                                                                  : "RSPT_SHADE_VARIANT names no instantiation with the sphere arm (generic-sphere, dynamic-sphere)");
    move = !volpath && !direct && !ao && !pixel_sampler && !s->has_animated && shade_move_k != nullptr && env_size("RSPT_MOVE", 1) != 0;
    // the first iteration that runs the MOVE kernel.  Iteration 0 reads a dense pixel-major queue whatever the schedule and its stores are dense too (every slot is
    // written): the slot-for-life kernel serves it (the MOVE form is 4 % slower there: 120 B of scratch against 36 at the same 168 VGPRs, profiles/r06_move_ab.txt),
    // and the first MOVE launch reads what it left in place
    move_first = (uint32_t)env_size("RSPT_MOVE_FROM", 1);
    if (!move) free_move();   // (213 GB at the default batch: the second set is not kept for renders that do not use it)
    ns = 1;  // samples per pixel per batch: largest power of two with n_pix * ns <= cap
    pix_per_batch = 1;
    for (;;) {
        ns = 1;
        while ((uint64_t)ns * 2 <= (uint64_t)d->spp && (uint64_t)n_pix * ns * 2 <= cap) ns *= 2;
        pix_per_batch = std::max<size_t>(1, std::min(n_pix, cap / ns));
        rc = ensure_paths(std::max<size_t>(pix_per_batch * ns, 1) * ao_n * dl_H * dl_R);
        if (rc == RSPT_OK && direct && !pixel_sampler && !dl_lane) rc = ensure_direct(g.cap);
        if (rc == RSPT_OK && volpath) rc = ensure_vol(g.cap);
        if (rc == RSPT_OK && move) rc = ensure_move(g.cap);
        if (rc == RSPT_OK) break;
        (void)hipGetLastError();  // out of memory: clear the sticky error and try half the batch
        free_paths();
        if (cap <= ((size_t)1 << 20)) return rc;
        cap /= 2;
    }
    return RSPT_OK;
}
int RenderRun::prepare() {
    int rc;
    // the per-lane directlighting forms: per-level texture rows, the light sample counts on the device, error / truncation words
    dl_tex_rows = RSPT_TEX_ROWS + (s->has_dynamic ? RSPT_DYN_ROWS : 0);
    dl_lanes = pixel_sampler ? n_blocks : pix_per_batch * ns;
    if (direct) {
        if (s->has_textures && (dl_lane || pixel_sampler)) {   // (the wavefront form over textures keeps its results in g.pb.tex; it cannot fall back to the per-lane form: that needs a specular lobe)
            if ((rc = dev_alloc(&dl_tex, (size_t)d->max_depth * dl_tex_rows * std::max<size_t>(dl_lanes, 1)))) return rc;
            temps.p.push_back(dl_tex);
            if (s->has_dynamic) {
                if ((rc = dev_alloc(&dl_dyn, (size_t)d->max_depth * std::max<size_t>(dl_lanes, 1)))) return rc;
                temps.p.push_back(dl_dyn);
            }
        }
        if (!pixel_sampler) {
            if ((rc = dev_alloc(&dl_words, 2))) return rc;
            temps.p.push_back(dl_words);
            if (d->n_light_samples && s->dev.n_lights) {
                if ((rc = dev_alloc(&dl_nls, s->dev.n_lights))) return rc;
                temps.p.push_back(dl_nls);
                HIP_TRY(hipMemcpy(dl_nls, d->n_light_samples, s->dev.n_lights * sizeof(int32_t), hipMemcpyHostToDevice));
            }
        }
    }
    nominal_iters = d->max_depth + 1;
    // a pass through a null-material surface costs a wavefront iteration without counting as a bounce (path.rs:109-116 has no limit
    // on them); the loop below runs until no path is left, and a scene that needs more than RSPT_NULL_PASSES extra iterations is
    // reported, not silently truncated
    max_iters = s->has_null_material ? nominal_iters + (uint32_t)env_size("RSPT_NULL_PASSES", 1024) : nominal_iters;
    if (volpath) HIP_TRY(hipMemsetAsync(g.vol.truncated, 0, sizeof(uint32_t), g.stream));
    // K7b: whole waves of one class (escaped | depth limit | material) for k_shade.  C3 stand-in (two materials): 1396 -> 1686 Msamples/s;
    // C2 (one material: only the escaped paths are separated): 423 -> 425
    // (measured with the specialised shade instantiations, profiles/r03_ab_shade.md: C3 stand-in — plastic statue on a matte ground — 1640 -> 1830
    //  Msamples/s with the bins; C2 — one material, only escaped paths to separate — 468 -> 456: the sort runs when lobe lists differ)
    shade_bins = env_size("RSPT_SHADE_BINS", s->shade_classes > 1 ? 1 : 0) != 0 && !ao && !direct && !volpath;
    if (shade_bins && (rc = ensure_bins(g.cap, max_iters + 10))) return rc;
    // iteration 0 (camera rays) arrives in pixel-major order — neighbouring slots, neighbouring pixels, mostly one material per wave already —
    // and has the longest queue of the batch: it is left unsorted (same box, alternating: C3 stand-in 1855 -> 1906 Msamples/s, textured
    // 1319 -> 1339; RSPT_BIN_FIRST=1 sorts it as before)
    bins_first = env_size("RSPT_BIN_FIRST", 0) != 0;
    if (s->has_instances && (rc = ensure_array(&g.hit_inst, &g.hit_inst_cap, volpath ? 2 * g.cap : g.cap))) return rc;   // volpath: second half = the hits of the shadow-ray segments
    // moving instances: every path keeps its ray time (the camera sample's), read where an instance's Transform is interpolated
    if (s->has_animated && (rc = ensure_array(&g.path_time, &g.time_cap, g.cap))) return rc;
    g.pb.time = s->has_animated ? g.path_time : nullptr;
    s->dev.ray_time = g.pb.time;
    s->dev.time_div = 1u;
    g.pb.fresh = 0u;
    // the realistic camera: a ray weight per sample, and the camera ray's differentials where a texture stage will want them
    if (realistic && ((rc = ensure_array(&g.ray_weight, &g.ray_weight_cap, g.cap)) || (s->has_textures && (rc = ensure_array(&g.cam_diff, &g.cam_diff_cap, 3 * g.cap))))) return rc;
    g.pb.ray_weight = realistic ? g.ray_weight : nullptr;
    g.pb.cam_diff = (realistic && s->has_textures) ? g.cam_diff : nullptr;
    g.pb.hit_inst = s->has_instances ? g.hit_inst : nullptr;
    g.vol.hit_inst_tr = (volpath && s->has_instances) ? g.hit_inst + g.cap : nullptr;
    if ((rc = ensure_array(&g.cnt, &g.n_cnt, max_iters + 10)) || (rc = ensure_array(&g.ovf, &g.ovf_cap, trace_can_overflow(s) ? 3 * g.cap : 1024)) || (rc = ensure_spill(pw_spill_threads())) ||
        (s->has_textures && (rc = ensure_tex_rows(s->has_dynamic)))) return rc;
    if (!g.totals) { if ((rc = dev_alloc(&g.totals, 8))) return rc; }
    HIP_TRY(hipMemsetAsync(g.totals, 0, 8 * sizeof(unsigned long long), g.stream));

    // LDS copy of the Sobol' matrices for k_shade: dimensions 0 .. 5 + 8 per bounce (+8 of read-ahead), index bits
    // 2*log2(resolution) + log2(spp) (lowdiscrepancy.rs:1014-1043); the checks above keep this under 64 KB
    sob_nd = 5u + 8u * (d->max_depth + 2u) + 8u;
    sob_bits = 2u * (uint32_t)rd.log2_res;
    for (int64_t v = d->spp; v > 1; v >>= 1) sob_bits++;
    sob_bits = std::min(52u, sob_bits + 1u);
    if ((size_t)sob_nd * sob_bits * 4 > 64 * 1024) return fail(RSPT_E_UNSUPPORTED, "max_depth %u x %u index bits exceed the LDS Sobol' table", d->max_depth, sob_bits);
    tgrid = trace_grid();
    if (getenv("RSPT_VERBOSE")) fprintf(stderr, "rspt: shade stage instantiation '%s'%s (scene features %#x)\n", shade_name, move ? ", moving path state" : "", s->shade_features);
    // one launch fills the chip once: as many 256-thread blocks per CU as the instantiation's registers and the LDS table allow
    int shade_blocks = 2;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&shade_blocks, reinterpret_cast<const void*>(shade_k), 256, sob_nd * sob_bits * sizeof(uint32_t)) != hipSuccess || shade_blocks < 1) {
        (void)hipGetLastError();
        shade_blocks = 2;
    }
    sgrid = grid_for((uint32_t)env_size("RSPT_SHADE_BLOCKS_PER_CU", (size_t)shade_blocks));
    if (getenv("RSPT_VERBOSE")) fprintf(stderr, "rspt: shade stage: %d blocks of 256 per CU\n", shade_blocks);
    // dynamic materials: one Built record per thread of the widest shade-stage launch (k_shade's grid; k_vol_shade runs grid_for(4))
    if (s->has_dynamic && (rc = ensure_dyn_built(std::max(sgrid, grid_for(8)) * 256u))) return rc;
    two_streams = env_size("RSPT_TRACE_STREAMS", 2) >= 2 && !counters;
    ev_fork = get_event(n_ev++); ev_join = get_event(n_ev++);
    ev_k0 = get_event(n_ev++); ev_k1 = get_event(n_ev++);
    HIP_TRY(hipEventRecord(ev_k0, g.stream));
    return RSPT_OK;
}
int RenderRun::finish(float* film_host, void* film_dev, float* li_host) {
    float4* out_dev = film_dev ? (float4*)film_dev : g.film_out;
    hipLaunchKernelGGL(k_film_resolve, dim3((uint32_t)((film_px + 255) / 256)), dim3(256), 0, g.stream, g.film_own, g.film_splat, out_dev, (uint32_t)film_px);
    if (d->film_reduce) {  // X1: sum of the ranks' films onto rank 0 (a sum, not a gather: tile pixel bounds overlap, film.rs:321-330)
        if (!rc_.comm) return fail(RSPT_E_INVALID, "film_reduce without a communicator (rspt_comm_init)");
        if ((uint32_t)rc_.world != shard_count || (uint32_t)rc_.rank != d->shard_index)
            return fail(RSPT_E_INVALID, "film_reduce: shard %u of %u does not match rank %d of %d", d->shard_index, shard_count, rc_.rank, rc_.world);
        hipError_t pe = hipStreamSynchronize(g.stream);   // a kernel fault of this rank must surface before the agreement, not inside the collective
        if (pe != hipSuccess) return fail(RSPT_E_HIP, "render failed: %s", hipGetErrorString(pe));
        int32_t any_failed = 0;
        if (int rc = film_reduce_agree(0, &any_failed)) return rc;
        if (any_failed) return fail(RSPT_E_PEER, "film_reduce: another rank of the communicator failed its render; no film was summed");
        RCCL_TRY(rc_.Reduce(out_dev, out_dev, film_px * 4, ncclFloat32, ncclSum, 0, rc_.comm, g.stream));
    }
    HIP_TRY(hipEventRecord(ev_k1, g.stream));
    HIP_TRY(hipGetLastError());
    if (film_host) HIP_TRY(hipMemcpyAsync(film_host, out_dev, film_px * sizeof(float4), hipMemcpyDeviceToHost, g.stream));
    if (li_host) HIP_TRY(hipMemcpyAsync(li_host, li_dev, film_px * (size_t)d->spp * 3 * sizeof(float), hipMemcpyDeviceToHost, g.stream));
    hipError_t se = hipStreamSynchronize(g.stream);
    if (se != hipSuccess) return fail(RSPT_E_HIP, "render failed: %s", hipGetErrorString(se));
    if (ld_lazy) {
        LightLazy lz;
        HIP_TRY(hipMemcpy(&lz, ld_lazy->lazy, sizeof lz, hipMemcpyDeviceToHost));
        if (lz.overflow) {
            LightLazy reset{0u, lz.n_rows, lz.max_rows, 0u};
            (void)hipMemcpy(ld_lazy->lazy, &reset, sizeof reset, hipMemcpyHostToDevice);
            return fail(RSPT_E_NOMEM, "spatial light distribution: more than %u voxels were touched; raise RSPT_LIGHT_TABLE_POOL_BYTES", lz.max_rows);
        }
    }
    return RSPT_OK;
}
int RenderRun::report(rspt_stats* stats, std::chrono::steady_clock::time_point t_start) {
    auto t_end = std::chrono::steady_clock::now();
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->t_render_s = std::chrono::duration<double>(t_end - t_start).count();
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev_k0, ev_k1));
        stats->t_kernels_s = ms * 1e-3;
        auto sum_ms = [](const std::vector<std::pair<hipEvent_t, hipEvent_t>>& v) {
            double t = 0;
            for (auto& e : v) { float m = 0; if (hipEventElapsedTime(&m, e.first, e.second) == hipSuccess) t += m; }
            return t;
        };
        stats->t_trace_s = sum_ms(trace_ev) * 1e-3;
        stats->t_trace_closest_s = sum_ms(kev[0]) * 1e-3; stats->t_trace_any_s = sum_ms(kev[1]) * 1e-3; stats->t_shade_s = sum_ms(kev[2]) * 1e-3;
        stats->launches_closest = kev[0].size(); stats->launches_any = kev[1].size();
        if (volpath) {  // paths vol.h cut because the sampler ran out of dimensions
            uint32_t tv = 0;
            HIP_TRY(hipMemcpy(&tv, g.vol.truncated, sizeof tv, hipMemcpyDeviceToHost));
            truncated += tv;
        }
        stats->truncated_paths = truncated;
        stats->samples = samples;
        stats->trace_launches = trace_launches;
        unsigned long long tot[8];
        HIP_TRY(hipMemcpy(tot, g.totals, sizeof tot, hipMemcpyDeviceToHost));
        stats->nan_samples = tot[5];
        if (volpath) { tot[3] = vol_rays; tot[4] = 0; }  // every volpath ray is a closest-hit ray (shadow rays walk segment by segment); counted from the queue lengths the host reads
        if (counters) {
            stats->nodes_visited = tot[0]; stats->tris_tested = tot[1];
            stats->rays_closest = tot[3]; stats->rays_any = tot[4];
            // B_alg = sum(32 N_node + 48 N_tri) + 96 R_closest + 72 R_any + 96 N_bounce + 32 per sample
            stats->alg_bytes = 32.0 * (double)tot[0] + 48.0 * (double)tot[1] + 96.0 * (double)tot[3] + 72.0 * (double)tot[4] + 96.0 * (double)tot[2] + 32.0 * (double)samples;
        }
    }
    return RSPT_OK;
}
