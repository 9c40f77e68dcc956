// The wavefront schedules of rspt_render: one batch of each integrator over the state of render_run.h, and the loop over the batches.
// Host code of librspt.hip, included there once inside its anonymous namespace.
// k_lane_dl<INST, ALPHA, ANIM, WH> by [whitted][0 plain | 1 object instances | 2 moving instances][alpha] (tu_decl.h: the ANIM forms exist with INST only)
#define RSPT_LANE_ROWS(WH) {{k_lane_dl<false, false, false, WH>, k_lane_dl<false, true, false, WH>}, {k_lane_dl<true, false, false, WH>, k_lane_dl<true, true, false, WH>}, {k_lane_dl<true, false, true, WH>, k_lane_dl<true, true, true, WH>}}
typedef void (*LaneKernel)(RSPT_LANE_ARGS);
const LaneKernel g_lane_dl[2][3][2] = {RSPT_LANE_ROWS(false), RSPT_LANE_ROWS(true)};
#undef RSPT_LANE_ROWS
    // the claimed voxels' rows: contributions of every light, the row's distribution, the table entries; returns how many were claimed
int RenderRun::build_claimed_rows(uint32_t* n_claimed) {
    LightLazy lz;
    HIP_TRY(hipMemcpyAsync(g.look, ld_lazy->lazy, sizeof lz, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    memcpy(&lz, g.look, sizeof lz);
    *n_claimed = lz.n_new;
    if (lz.overflow) return fail(RSPT_E_NOMEM, "spatial light distribution: more than %u voxels were touched; raise RSPT_LIGHT_TABLE_POOL_BYTES", lz.max_rows);
    if (lz.n_new == 0) return RSPT_OK;
    const uint32_t lgrid = grid_for(4);
    hipLaunchKernelGGL(k_ld_contrib_list, dim3(lgrid), dim3(256), 0, g.stream, s->dev, ld.nvox[0], ld.nvox[1], ld.nvox[2], ld_lazy->lazy, ld_lazy->new_list, ld_lazy->func);
    hipLaunchKernelGGL(k_ld_build_list, dim3(lgrid), dim3(256), 0, g.stream, s->dev.n_lights, ld_lazy->lazy, ld_lazy->new_list, ld_lazy->func, ld_lazy->cdf, ld_lazy->func_int, ld_lazy->table);
    hipLaunchKernelGGL(k_ld_commit, dim3(1), dim3(1), 0, g.stream, ld_lazy->lazy);
    return RSPT_OK;
}
// ---- one batch of each integrator (the wavefront schedules); `it` leaves with the number of queue-counter records used ----
// Which kernel serves this scene's shadow rays (trace_w4q.h; launch_trace_v): measured once per scene, by the first shadow-ray launch of a batch of >= 2^22 paths — both kernels
// run on the same rays (their flags are identical), the faster one is kept in rspt_scene_s::any_q_choice.  Returns 1 if it made the launch (twice), 0 if there was nothing to
// measure (the caller launches as usual), -code on an error.
int RenderRun::tune_any(uint32_t batch_n, TraceCall c) {
    if (!s->w4q || s->any_q_choice >= 0 || getenv("RSPT_ANY_Q") || counters || batch_n < (1u << 22) || env_size("RSPT_ANY_Q_TUNE", 1) == 0) return 0;
    hipEvent_t t0 = get_event(n_ev++), t1 = get_event(n_ev++), t2 = get_event(n_ev++);
    if (hipEventRecord(t0, g.stream) != hipSuccess) return RSPT_E_HIP;
    c.force_any_q = 0;
    launch_trace<true, 0>(tgrid, s, c);
    (void)hipEventRecord(t1, g.stream);
    (void)hipMemsetAsync(c.cursor, 0, sizeof(uint32_t), g.stream);   // (the persistent kernel's fetch cursor: the second run starts over)
    c.force_any_q = 1;
    launch_trace<true, 0>(tgrid, s, c);
    (void)hipEventRecord(t2, g.stream);
    if (hipEventSynchronize(t2) != hipSuccess) return RSPT_E_HIP;
    float ms_plain = 0.0f, ms_q = 0.0f;
    (void)hipEventElapsedTime(&ms_plain, t0, t1);
    (void)hipEventElapsedTime(&ms_q, t1, t2);
    s->any_q_choice = ms_q < ms_plain ? 1 : 0;
    if (getenv("RSPT_VERBOSE")) fprintf(stderr, "rspt: shadow rays of this scene: k_trace_w4<any> %.2f ms, k_trace_w4q %.2f ms on the same launch -> %s\n", ms_plain, ms_q, s->any_q_choice ? "the quantised records" : "the plain records");
    return 1;
}
// Which kernel serves this scene's camera-ray launches (trace_packet.h, trace_frustum.h, trace_bundle.h; launch_trace_v): measured once per scene, by the first camera launch of >= 2^22 rays of a
// path render — the five candidates (four extra launches, once per scene) run on the same rays (their hit records are identical, and the launch only writes them), the fastest one is kept in rspt_scene_s::camera_pk_choice.
// RSPT_CAMERA_PACKET_TUNE=0 skips the measurement (the scene stays on k_trace_w4).  Returns as tune_any does.
int RenderRun::tune_camera(uint32_t batch_n, TraceCall c) {
    if (s->camera_pk_choice >= 0 || getenv("RSPT_CAMERA_PACKET") || counters || d->integrator != RSPT_INTEGRATOR_PATH || batch_n < (1u << 22) || env_size("RSPT_CAMERA_PACKET_TUNE", 1) == 0) return 0;
    if (!camera_packet_ok(s, env_size("RSPT_TRACE_KERNEL", 2), (c.xcd_cursors && env_size("RSPT_XCD_DEAL", 0) != 0) ? c.xcd_cursors : nullptr)) return 0;
    constexpr int NK = 5;
    hipEvent_t t[NK + 1];
    for (int k = 0; k <= NK; k++) t[k] = get_event(n_ev++);
    if (hipEventRecord(t[0], g.stream) != hipSuccess) return RSPT_E_HIP;
    for (int k = 0; k < NK; k++) {
        if (k) (void)hipMemsetAsync(c.cursor, 0, sizeof(uint32_t), g.stream);   // (the persistent kernel's fetch cursor: the next run starts over)
        c.force_camera_pk = k;
        launch_trace<false, 0>(tgrid, s, c);
        (void)hipEventRecord(t[k + 1], g.stream);
    }
    if (hipEventSynchronize(t[NK]) != hipSuccess) return RSPT_E_HIP;
    float ms[NK] = {};
    for (int k = 0; k < NK; k++) (void)hipEventElapsedTime(&ms[k], t[k], t[k + 1]);
    int pick = 0;
    for (int k = 1; k < NK; k++) if (ms[k] < ms[pick]) pick = k;
    s->camera_pk_choice = pick;
    static const char* const names[NK] = {"per-lane walks", "64-ray packets", "64-ray packets, one frustum test per record", "bundles of two packets, one frustum walk each",
                                          "bundles of four packets, one frustum walk each"};
    if (getenv("RSPT_VERBOSE"))
        fprintf(stderr, "rspt: camera rays of this scene: k_trace_w4 %.2f ms, k_trace_w4pk %.2f ms, k_trace_w4pf %.2f ms, k_trace_w4pb<2> %.2f ms, k_trace_w4pb<4> %.2f ms on the same launch -> %s\n",
                ms[0], ms[1], ms[2], ms[3], ms[4], names[pick]);
    return 1;
}
int RenderRun::batch_volpath(const Batch& bt, uint32_t& it) {  // VolPathIntegrator::li (vol.h): the continuation queue doubles as the list of live paths
    int rc;
    const uint32_t dgrid = grid_for(4);
    const uint32_t null_passes = (uint32_t)env_size("RSPT_NULL_PASSES", 1024);
    // LDS table: 10 dimensions per counted pass, 2 per pass through a medium boundary (room for 64 of those), 8 of read-ahead;
    // a path that needs more is cut and counted (rspt_stats.truncated_paths); the reference's own limit is 1024
    const uint32_t vnd = std::min(1024u, 5u + 10u * (d->max_depth + 2u) + 128u) + 8u;
    if ((size_t)vnd * sob_bits * 4 > 64 * 1024) return fail(RSPT_E_UNSUPPORTED, "volpath: max_depth %u x %u index bits exceed the LDS Sobol' table", d->max_depth, sob_bits);
    const uint32_t vlimit = halton ? vol_dim_limit : std::min(1024u, vnd - 8u);
    hipLaunchKernelGGL(k_vol_init, dim3((bt.n + 255) / 256), dim3(256), 0, g.stream, g.vol, bt.n);
    // counters: g.cnt[0 / 1] = the continuation queue of this / the next pass, g.cnt[2 / 3] = the shadow-ray segments
    uint32_t live = bt.n;
    for (uint32_t pass = 0; live > 0; pass++) {
        const int par = pass & 1;
        QueueCounts* cur = &g.cnt[par];
        QueueCounts* nxt = &g.cnt[par ^ 1];
        HIP_TRY(hipMemsetAsync(nxt, 0, sizeof(QueueCounts), g.stream));
        HIP_TRY(hipMemsetAsync(&g.cnt[2], 0, sizeof(QueueCounts), g.stream));
        ev_open(0, 0);
        launch_trace<false, 0>(tgrid, s, closest_call(g.pb, g.q[par][1], &cur->closest, &cur->cursor_closest, counters));
        ev_close(0, 0);
        trace_launches++;
        vol_rays += live;
        ev_open(2, 0);
        if (s->has_textures) hipLaunchKernelGGL(k_texture, dim3(dgrid), dim3(256), 0, g.stream, s->dev, s->tex, rd, g.pb, g.q[par][1], &cur->closest, (const uint32_t*)nullptr, (const BinInfo*)nullptr);
        if (ld.lazy) HIP_TRY(hipMemsetAsync(&cur->active, 0, sizeof(uint32_t), g.stream));   // (k_raygen leaves the batch size there; volpath itself does not use the active queues)
        hipLaunchKernelGGL(s->has_dynamic ? k_vol_shade<true> : k_vol_shade<false>, dim3(dgrid), dim3(256), halton ? 0 : vnd * sob_bits * sizeof(uint32_t), g.stream, s->dev, ld, rd, g.pb, g.vol, g.q[par][1], &cur->closest,
                           g.q[par ^ 1][1], &nxt->closest, g.q[0][2], &g.cnt[2].closest, vlimit, vnd, sob_bits, ld.lazy ? g.q[par][0] : (uint32_t*)nullptr, &cur->active);
        // on-demand light voxels: paths whose voxel had no row were put back (q[par][0], counted in cur->active, zero until here); build the rows, run those paths
        for (uint32_t round = 0; ld.lazy; round++) {
            uint32_t claimed = 0;
            if ((rc = build_claimed_rows(&claimed))) return rc;
            HIP_TRY(hipMemcpyAsync(g.look, cur, sizeof(QueueCounts), hipMemcpyDeviceToHost, g.stream));
            HIP_TRY(hipStreamSynchronize(g.stream));
            const uint32_t n_retry = g.look[0].active;
            if (n_retry == 0) break;
            if (round > 64) return fail(RSPT_E_UNSUPPORTED, "volpath: on-demand light voxels did not settle in 64 rounds (not a device fault: the caller keeps its CPU loop, or asks for the eager table)");
            // the retry queue becomes the input (copied to the other parity's active queue, which volpath does not use either), its counter starts again
            HIP_TRY(hipMemcpyAsync(g.q[par ^ 1][0], g.q[par][0], (size_t)n_retry * sizeof(uint32_t), hipMemcpyDeviceToDevice, g.stream));
            HIP_TRY(hipMemcpyAsync(&cur->any, &cur->active, sizeof(uint32_t), hipMemcpyDeviceToDevice, g.stream));   // (cur->any: the retry run's input length)
            HIP_TRY(hipMemsetAsync(&cur->active, 0, sizeof(uint32_t), g.stream));
            hipLaunchKernelGGL(s->has_dynamic ? k_vol_shade<true> : k_vol_shade<false>, dim3(dgrid), dim3(256), halton ? 0 : vnd * sob_bits * sizeof(uint32_t), g.stream, s->dev, ld, rd, g.pb, g.vol,
                               g.q[par ^ 1][0], &cur->any, g.q[par ^ 1][1], &nxt->closest, g.q[0][2], &g.cnt[2].closest, vlimit, vnd, sob_bits, g.q[par][0], &cur->active);
        }
        ev_close(2, 0);
        // VisibilityTester::tr: segments until every shadow ray has arrived or is blocked
        // (the first two segments are launched without looking at the queue: most shadow rays cross at most one boundary, an
        //  empty launch costs microseconds, a look costs a stream synchronisation; the look that follows also brings the
        //  next pass's path count)
        QueueCounts* look = g.look;   // (pinned: see Ctx::look)
        bool have_live = false;
        for (uint32_t seg = 0;; seg++) {
            QueueCounts* tc = &g.cnt[2 + (seg & 1u)];
            QueueCounts* tn = &g.cnt[2 + ((seg + 1u) & 1u)];
            QueueCounts c{};
            c.closest = live;   // upper bound while not looking (every live path has at most one shadow ray)
            const bool looked = seg >= 2 || counters;   // (the counting pass wants every queue length)
            if (looked) {
                HIP_TRY(hipMemcpyAsync(look, g.cnt, 4 * sizeof(QueueCounts), hipMemcpyDeviceToHost, g.stream));
                HIP_TRY(hipStreamSynchronize(g.stream));
                c = look[2 + (seg & 1u)];
                have_live = true;
                if (c.closest == 0) break;
            }
            if (seg > null_passes) { truncated += c.closest; break; }
            HIP_TRY(hipMemsetAsync(tn, 0, sizeof(QueueCounts), g.stream));
            ev_open(1, 0);
            // (queue entries without the MIS flag over the shadow rays' own arrays, so that the hit's instance is recorded too)
            TraceCall sc = closest_call(g.pb, g.q[seg & 1u][2], &tc->closest, &tc->cursor_closest, counters);
            sc.ra = g.pb.ray_mis; sc.oa = g.pb.hit_mis;
            sc.inst_out = g.vol.hit_inst_tr ? g.hit_inst + g.cap : nullptr;
            launch_trace<false, 0>(tgrid, s, sc);
            ev_close(1, 0);
            trace_launches++;
            if (looked) vol_rays += c.closest;
            hipLaunchKernelGGL(s->has_animated ? k_vol_tr<true> : k_vol_tr<false>, dim3(dgrid), dim3(256), 0, g.stream, s->dev, g.pb, g.vol, g.q[seg & 1u][2], &tc->closest, g.q[(seg + 1u) & 1u][2], &tn->closest);
        }
        if (!have_live) {
            HIP_TRY(hipMemcpyAsync(look, g.cnt, 4 * sizeof(QueueCounts), hipMemcpyDeviceToHost, g.stream));
            HIP_TRY(hipStreamSynchronize(g.stream));
        }
        live = look[par ^ 1].closest;
        if (live && pass >= nominal_iters + null_passes) { truncated += live; break; }
    }
    it = 4;
    return RSPT_OK;
}
int RenderRun::batch_direct(const Batch& bt, uint32_t& it) {  // DirectLightingIntegrator::li (direct.h): specular tree, dimension assignment, light rounds, gather
    const uint32_t nl = s->dev.n_lights, H = dl_H, md = d->max_depth;
    const bool all = d->direct_strategy == RSPT_DIRECT_SAMPLE_ALL;
    const uint32_t n_arrays = (all && !whitted) ? 2u * md * nl : 0u;
    // the sample arrays are filled for every pixel sample whether a node uses them or not (GlobalSampler::start_pixel), so they must fit;
    // the regular stream behind them is checked per camera sample by k_dl_assign against what each tree really draws
    const uint32_t dim_limit = halton ? vol_dim_limit + 1u : 1024u;
    if (5ull + 2ull * n_arrays > dim_limit)
        return fail(RSPT_E_UNSUPPORTED, "%s: %u sample arrays exceed the sampler's %u dimensions", dl_name, n_arrays, dim_limit);
    DlBuf dl = g.dl;
    dl.H = H; dl.levels = dl_levels;
    s->dev.time_div = H;   // node h of camera sample s lives in slot s * H + h: its rays carry the sample's time (moving instances); estimate rays: below
    struct TimeDivReset { rspt_scene_s* s; ~TimeDivReset() { s->dev.time_div = 1u; } } time_div_reset{s};
    const size_t n_slots = (size_t)bt.n * H;
    // virtual slots of the estimates (direct.h DlBuf::vs / vr): planes of n_slots, unless a moving instance needs slot -> camera sample by one division (RSPT_DL_PLANES=0: A/B)
    const bool dl_planes = !s->has_animated && env_size("RSPT_DL_PLANES", 1) != 0;
    dl.vs = dl_planes ? 1u : dl_R; dl.vr = dl_planes ? (uint32_t)n_slots : 1u;
    if (s->has_textures) HIP_TRY(hipMemsetAsync(g.pb.state, 0, n_slots * sizeof(uint32_t), g.stream));   // (ST_NO_DIFF marks of k_dl_hit, read by k_dl_texture)
    HIP_TRY(hipMemsetAsync(dl.le_kind, 0, n_slots * sizeof(float4), g.stream));
    HIP_TRY(hipMemsetAsync(dl.l_all, 0, n_slots * sizeof(float4), g.stream));
    HIP_TRY(hipMemsetAsync(dl.ld_acc, 0, n_slots * sizeof(float4), g.stream));
    HIP_TRY(hipMemsetAsync(dl.error, 0, sizeof(uint32_t), g.stream));
    // the camera rays were left in ray_cont[sample]; node slots overlay that array, so move them aside first
    HIP_TRY(hipMemcpyAsync(g.pb.ray_sh, g.pb.ray_cont, (size_t)bt.n * sizeof(rspt_ray), hipMemcpyDeviceToDevice, g.stream));
    // counters: g.cnt[level].closest = nodes of the level, .any = re-trace queue; rounds use g.cnt[md + 1 ..]
    auto level_q = [&](uint32_t l) { return g.dl_queue + (size_t)bt.n * ((1u << l) - 1u); };
    hipLaunchKernelGGL(k_dl_init, dim3((bt.n + 255) / 256), dim3(256), 0, g.stream, bt, g.pb, dl, g.pb.ray_sh, level_q(0), &g.cnt[0].closest);
    const uint32_t dgrid = grid_for(4);
    for (uint32_t l = 0; l < dl_levels; l++) {
        const uint32_t* queue = level_q(l);
        const uint32_t* qcount = &g.cnt[l].closest;
        for (uint32_t round = 0;; round++) {
            QueueCounts* rc_ = &g.cnt[md + 1 + (round & 1u)];  // re-trace queue of this round (null-BSDF hits), double buffered
            HIP_TRY(hipMemsetAsync(rc_, 0, sizeof(QueueCounts), g.stream));
            HIP_TRY(hipMemsetAsync((void*)&g.cnt[l].cursor_closest, 0, 3 * sizeof(uint32_t), g.stream));
            ev_open(0, 0);
            launch_trace<false, 0>(tgrid, s, closest_call(g.pb, queue, qcount, round == 0 ? &g.cnt[l].cursor_closest : &g.cnt[md + 1 + ((round - 1) & 1u)].cursor_closest, false));
            ev_close(0, 0);
            trace_launches++;
            ev_open(2, 0);
            hipLaunchKernelGGL(k_dl_hit, dim3(dgrid), dim3(256), 0, g.stream, s->dev, rd, g.pb, dl, queue, qcount, g.q[round & 1u][0], &rc_->closest,
                               level_q(l + 1 < dl_levels ? l + 1 : l), &g.cnt[l + 1].closest, l);
            ev_close(2, 0);
            if (!s->has_null_material) break;
            HIP_TRY(hipMemcpyAsync(g.look, rc_, sizeof(QueueCounts), hipMemcpyDeviceToHost, g.stream));
            HIP_TRY(hipStreamSynchronize(g.stream));
            const QueueCounts c = g.look[0];
            if (c.closest == 0) break;
            if (round >= env_size("RSPT_NULL_PASSES", 1024)) { truncated += c.closest; break; }
            queue = g.q[round & 1u][0];
            qcount = &rc_->closest;
        }
    }
    hipLaunchKernelGGL(whitted ? k_dl_assign<true> : k_dl_assign<false>, dim3((bt.n + 255) / 256), dim3(256), 0, g.stream, bt, dl, nl, n_arrays, all ? 1u : 0u, md, dim_limit);
    if (s->has_textures)   // (dl_tex_wave: one level, the roots) the texture stage in front of the estimates
        for (uint32_t l = 0; l < dl_levels; l++)
            hipLaunchKernelGGL(k_dl_texture, dim3(dgrid), dim3(256), 0, g.stream, s->dev, s->tex, rd, g.pb, dl, level_q(l), &g.cnt[l].closest);
    if (nl && dl_one_round) {   // every estimate of a level's nodes in one round: 4 launches per level (direct.h k_dl_nee_all)
        QueueCounts* rc_ = &g.cnt[md + 3];
        for (uint32_t l = 0; l < dl_levels; l++) {
            HIP_TRY(hipMemsetAsync(rc_, 0, sizeof(QueueCounts), g.stream));
            ev_open(2, 0);
            // the estimate kernel per feature set, as k_shade<F>: scenes of Lambert / microfacet-reflection lobes under area lights without instances (C1 - C3) take the
            // narrow build (RSPT_DL_VARIANT=generic forces the other)
            constexpr uint32_t DLV_PLASTIC = SV_PLASTIC | SF_SOBOL | SF_HALTON;
            const bool dl_narrow = (s->shade_features & ~DLV_PLASTIC) == 0 && !(getenv("RSPT_DL_VARIANT") && !strcmp(getenv("RSPT_DL_VARIANT"), "generic"));
            const size_t dl_waves = env_size("RSPT_DL_WAVES", RSPT_DL_WAVES_DEFAULT);   // 3: the narrow build forced to 3 waves per SIMD
            // the Sobol' tables the estimates read, in LDS (direct.h DlSob): the sample arrays' dimensions 5 .. 5 + 2 n_arrays and what the regular stream adds behind them,
            // for indices of 2 log2_res + log2(spp x the longest array) bits; cut to 40 KB (the rest falls back to the global walks); RSPT_DL_LDS_SOBOL=0: as before
            uint32_t dsn = 0, dsb = 0;
            if (!halton && env_size("RSPT_DL_LDS_SOBOL", 1) != 0) {
                uint64_t longest = 1;
                for (uint32_t j = 0; all && d->n_light_samples && j < nl; j++) longest = std::max<uint64_t>(longest, (uint64_t)std::max<int32_t>(d->n_light_samples[j], 1));
                dsb = 2u * (uint32_t)rd.log2_res + 1u;
                for (uint64_t v = (uint64_t)std::max<int64_t>(d->spp, 1) * longest; v > 1; v >>= 1) dsb++;
                dsb = std::min(52u, dsb);
                dsn = std::min<uint32_t>(1024u, 5u + 2u * n_arrays + 8u * (md + 2u));
                if (whitted) dsn = (uint32_t)std::min<uint64_t>(1024u, 5u + (2ull * nl + 4u) * ((1ull << dl_levels) - 1u));   // the deepest tree's stream
                dsn = std::min<uint32_t>(dsn, (40u * 1024u) / (4u * dsb));
                if (dsn < 16u) dsn = dsb = 0;
            }
            // the lights and the area lights' triangle records in LDS too (direct.h DlSob::lights: their loads must not queue behind the estimates' stores); the count
            // rides in bits 16.. of the index-bits argument.  RSPT_DL_LDS_LIGHTS=0: from global memory as before
            const uint32_t dll = (nl <= DL_LDS_LIGHTS && env_size("RSPT_DL_LDS_LIGHTS", 1) != 0) ? nl : 0u;
            const size_t dl_lds = (dll ? (((size_t)dll * (48 + sizeof(rspt_light)) + 7) / 8) * 8 : 0) + (dsn ? 104 * sizeof(uint64_t) + (size_t)dsn * dsb * sizeof(uint32_t) : 0);
            dsb |= dll << 16;
            if (whitted)   // (WhittedIntegrator: one estimate per light, direct.h dl_nee_all<F, true>)
                hipLaunchKernelGGL(dl_narrow ? k_wh_nee_all<DLV_PLASTIC> : k_wh_nee_all<SF_ALL>, dim3(dgrid), dim3(256), dl_lds, g.stream, s->dev, rd, bt, g.pb, dl, g.pix_list, level_q(l), &g.cnt[l].closest,
                                   (const int32_t*)nullptr, dl_R, 0u, 1u, g.q[0][2], &rc_->any, g.q[0][1], &rc_->closest, dsn, dsb, dim_limit);
            else
            hipLaunchKernelGGL(dl_narrow ? (dl_waves == 3 ? k_dl_nee_all_w<DLV_PLASTIC, 3> : k_dl_nee_all<DLV_PLASTIC>) : k_dl_nee_all<SF_ALL>, dim3(dgrid), dim3(256), dl_lds, g.stream, s->dev, rd, bt, g.pb, dl, g.pix_list, level_q(l), &g.cnt[l].closest, (const int32_t*)dl_nls, dl_R,
                               n_arrays, all ? 1u : 0u, g.q[0][2], &rc_->any, g.q[0][1], &rc_->closest, dsn, dsb);
            ev_close(2, 0);
            ev_open(1, 0);
            s->dev.time_div = H * dl_R;   // estimate r of node slot n sits in virtual slot n * R + r
            {
                const TraceCall ta = any_call(g.pb, g.q[0][2], &rc_->any, &rc_->cursor_any, false);
                const int tuned = tune_any(bt.n, ta);   // (the scene's first large shadow-ray launch measures the two kernels)
                if (tuned < 0) return fail(tuned, "the shadow-ray kernel measurement failed");
                if (!tuned) launch_trace<true, 0>(tgrid, s, ta);
            }
            ev_close(1, 0);
            ev_open(0, 0);
            launch_trace<false, 0>(tgrid, s, closest_call(g.pb, g.q[0][1], &rc_->closest, &rc_->cursor_closest, false));
            s->dev.time_div = H;
            ev_close(0, 0);
            trace_launches += 2;
            hipLaunchKernelGGL(k_dl_nee_resolve_all, dim3(dgrid), dim3(256), 0, g.stream, s->dev, g.pb, dl, level_q(l), &g.cnt[l].closest, (const int32_t*)dl_nls, dl_R, n_arrays, all ? 1u : 0u);
        }
    } else if (nl) {
        QueueCounts* rc_ = &g.cnt[md + 3];
        for (uint32_t l = 0; l < dl_levels; l++) {
            const uint32_t n_lights_round = all ? nl : 1u;
            for (uint32_t j = 0; j < n_lights_round; j++) {
                const uint32_t n_j = all ? (uint32_t)(d->n_light_samples ? d->n_light_samples[j] : 1) : 1u;
                for (uint32_t kk = 0; kk < n_j; kk++) {
                    HIP_TRY(hipMemsetAsync(rc_, 0, sizeof(QueueCounts), g.stream));
                    ev_open(2, 0);
                    hipLaunchKernelGGL(k_dl_nee, dim3(dgrid), dim3(256), 0, g.stream, s->dev, rd, bt, g.pb, dl, g.pix_list, level_q(l), &g.cnt[l].closest, j, kk, n_j,
                                       n_arrays, all ? 1u : 0u, g.q[0][2], &rc_->any, g.q[0][1], &rc_->closest);
                    ev_close(2, 0);
                    ev_open(1, 0);
                    launch_trace<true, 0>(tgrid, s, any_call(g.pb, g.q[0][2], &rc_->any, &rc_->cursor_any, false));
                    ev_close(1, 0);
                    ev_open(0, 0);
                    launch_trace<false, 0>(tgrid, s, closest_call(g.pb, g.q[0][1], &rc_->closest, &rc_->cursor_closest, false));
                    ev_close(0, 0);
                    trace_launches += 2;
                    hipLaunchKernelGGL(k_dl_nee_resolve, dim3(dgrid), dim3(256), 0, g.stream, s->dev, g.pb, dl, level_q(l), &g.cnt[l].closest, j, kk, n_j, n_arrays, all ? 1u : 0u);
                }
            }
        }
    }
    hipLaunchKernelGGL(k_dl_gather, dim3((bt.n + 255) / 256), dim3(256), 0, g.stream, bt, g.pb, dl, nl, md);
    uint32_t dl_err = 0;
    HIP_TRY(hipMemcpyAsync(&dl_err, dl.error, sizeof dl_err, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    if (dl_err == 1u) return RSPT_DL_RETRY_LANE;   // a material with several specular lobes of one kind: the lobe choice depends on a sample value, the tree cannot be traced ahead
    if (dl_err == 3u) return fail(RSPT_E_HIP, "%s: a specular bounce in a scene classified as having none", dl_name);
    if (dl_err) return fail(RSPT_E_UNSUPPORTED, "%s: a camera sample draws more than the sampler's %u dimensions (the reference panics there, sobol.rs:119-124)", dl_name, dim_limit);
    it = md + 4;
    return RSPT_OK;
}
int RenderRun::batch_direct_lane(const Batch& bt, uint32_t& it) {  // the same integrator, one lane per camera sample (lane_serial.h)
    const uint32_t nl = s->dev.n_lights, md = d->max_depth;
    const bool all = d->direct_strategy == RSPT_DIRECT_SAMPLE_ALL;
    const uint32_t n_arrays = (all && !whitted) ? 2u * md * nl : 0u;
    const uint32_t dim_limit = halton ? vol_dim_limit + 1u : 1024u;
    if (5ull + 2ull * n_arrays > dim_limit)
        return fail(RSPT_E_UNSUPPORTED, "%s: %u sample arrays exceed the sampler's %u dimensions", dl_name, n_arrays, dim_limit);
    HIP_TRY(hipMemsetAsync(dl_words, 0, 2 * sizeof(uint32_t), g.stream));
    const LaneDesc ln{all ? dl_nls : nullptr, n_arrays, all ? 1u : 0u, dim_limit, dl_tex, (uint32_t)dl_lanes, dl_tex_rows, dl_dyn,
                      s->has_null_material ? (uint32_t)env_size("RSPT_NULL_PASSES", 1024) : 0u, dl_words, dl_words + 1};
    const dim3 lgrid((bt.n + 63u) / 64u);
    ev_open(2, 0);
    // (moving instances, round 6: the walk interpolates the instances it enters at the sample's ray time, pb.time; whitted: lane_serial.h k_lane_dl<.., WH>)
    hipLaunchKernelGGL(g_lane_dl[whitted][s->has_animated ? 2 : (s->has_instances ? 1 : 0)][s->has_alpha], lgrid, dim3(64), 0, g.stream, s->dev, s->tex, ld, rd, bt, g.pb, g.pix_list, ln);
    ev_close(2, 0);
    uint32_t w[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(w, dl_words, sizeof w, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    if (w[0]) return fail(RSPT_E_UNSUPPORTED, "%s: a camera sample draws more than the sampler's %u dimensions (the reference panics there, sobol.rs:119-124)", dl_name, dim_limit);
    truncated += w[1];
    it = 1;
    return RSPT_OK;
}
int RenderRun::batch_ao(const Batch& bt, uint32_t& it) {  // AOIntegrator::li: closest hit, n shadow rays per hit, sum of the unoccluded terms
    hipEvent_t e0 = get_event(n_ev++), e1 = get_event(n_ev++), e2 = get_event(n_ev++), e3 = get_event(n_ev++);
    HIP_TRY(hipEventRecord(e0, g.stream));
    ev_open(0, 0);
    launch_trace<false, 0>(tgrid, s, closest_call(g.pb, g.q[0][1], &g.cnt[0].closest, &g.cnt[0].cursor_closest, counters));
    ev_close(0, 0);
    HIP_TRY(hipEventRecord(e1, g.stream));
    hipLaunchKernelGGL(s->has_quadrics ? k_ao_spawn_quad : s->has_spheres ? k_ao_spawn_sph : (s->has_animated ? k_ao_spawn<true> : k_ao_spawn<false>), dim3((bt.n + 255) / 256), dim3(256), 0, g.stream, s->dev, rd, bt, g.pb, g.pix_list, ao_n, d->ao_cos_sample, g.q[0][2], &g.cnt[1]);
    HIP_TRY(hipEventRecord(e2, g.stream));
    ev_open(1, 0);
    s->dev.time_div = ao_n;   // shadow ray k of camera sample i sits in slot i * n + k: its Ray.time is the sample's (moving instances)
    launch_trace<true, 0>(tgrid, s, any_call(g.pb, g.q[0][2], &g.cnt[1].any, &g.cnt[1].cursor_any, counters));
    s->dev.time_div = 1u;
    ev_close(1, 0);
    HIP_TRY(hipEventRecord(e3, g.stream));
    trace_ev.push_back({e0, e1}); trace_ev.push_back({e2, e3});
    trace_launches += 2;
    hipLaunchKernelGGL(k_ao_resolve, dim3((bt.n + 255) / 256), dim3(256), 0, g.stream, bt, g.pb, ao_n);
    it = 2;
    return RSPT_OK;
}
int RenderRun::batch_path(const Batch& bt, uint32_t& it) {  // PathIntegrator::li: trace (closest || any) -> [light voxels] -> [bins] -> [textures] -> shade, per bounce
    for (;;) {
        const int par = it & 1;
        if (it > 0) g.pb.fresh = 0u;   // (PathBuf travels by value: the first launches of the batch have carried the flag k_raygen ran with)
        const PathBuf P = move ? move_pathbuf(it, move_first) : g.pb;   // MOVE: the set this iteration reads (written by the previous one's shade launch) and the set it writes
        hipEvent_t e0 = get_event(n_ev++), e1 = get_event(n_ev++);
        HIP_TRY(hipEventRecord(e0, g.stream));
        // the shadow-ray launch does not depend on the closest-hit launch: on a second stream its tail (a few
        // long rays on an otherwise idle chip) overlaps the other launch
        int any_lane = (it > 0 && two_streams) ? 1 : 0;
        bool any_done = false;
        TraceCall ta = any_call(P, g.q[par][2], &g.cnt[it].any, &g.cnt[it].cursor_any, counters);
        ta.xcd_cursors = g.cnt[it].xcd_any;
        if (it == 1) {   // (the scene's first large shadow-ray launch measures the two kernels: tune_any above)
            ev_open(1, 0);
            const int tuned = tune_any(bt.n, ta);
            ev_close(1, 0);
            if (tuned < 0) return fail(tuned, "the shadow-ray kernel measurement failed");
            if (tuned) { any_done = true; any_lane = 0; }
        }
        if (any_lane) {
            HIP_TRY(hipEventRecord(ev_fork, g.stream));
            HIP_TRY(hipStreamWaitEvent(g.stream2, ev_fork, 0));
            ev_open(1, 1);
            ta.lane = 1;
            launch_trace<true, 0>(tgrid, s, ta);
            ev_close(1, 1);
            HIP_TRY(hipEventRecord(ev_join, g.stream2));
        }
        ev_open(0, 0);
        TraceCall tc = closest_call(P, g.q[par][1], &g.cnt[it].closest, &g.cnt[it].cursor_closest, counters);
        tc.xcd_cursors = g.cnt[it].xcd_closest;
        tc.camera_launch = it == 0;
        int cam_tuned = 0;
        if (it == 0 && (cam_tuned = tune_camera(bt.n, tc)) < 0) return fail(cam_tuned, "the camera-ray kernel measurement failed");   // (the scene's first large camera launch measures the two kernels)
        if (!cam_tuned) launch_trace<false, 0>(tgrid, s, tc);
        ev_close(0, 0);
        if (any_lane) HIP_TRY(hipStreamWaitEvent(g.stream, ev_join, 0));
        else if (it > 0 && !any_done) {
            ev_open(1, 0);
            launch_trace<true, 0>(tgrid, s, ta);
            ev_close(1, 0);
        }
        HIP_TRY(hipEventRecord(e1, g.stream));
        trace_ev.push_back({e0, e1});
        trace_launches += it > 0 ? 2 : 1;
        ev_open(2, 0);
        const bool bins_now = shade_bins && (it > 0 || bins_first);
        if (bins_now) {  // K7b: whole waves of one class for k_shade
            const uint32_t bgrid = hinted_grid(queue_hint, grid_for(4), 256);
            hipLaunchKernelGGL(k_bin_count, dim3(bgrid), dim3(256), 0, g.stream, s->dev, P, d->max_depth, g.q[par][0], &g.cnt[it], g.bin_keys, &g.bin_info[it]);
            hipLaunchKernelGGL(k_bin_starts, dim3(1), dim3(64), 0, g.stream, &g.bin_info[it], g.q_sorted);
            hipLaunchKernelGGL(k_bin_scatter, dim3(bgrid), dim3(256), 0, g.stream, g.q[par][0], &g.cnt[it], g.bin_keys, &g.bin_info[it], g.q_sorted);
        }
        if (ld_lazy && d->integrator == RSPT_INTEGRATOR_PATH) {
            const uint32_t lgrid = hinted_grid(queue_hint, grid_for(4), 256);
            hipLaunchKernelGGL(k_ld_mark, dim3(lgrid), dim3(256), 0, g.stream, s->dev, ld, P, d->max_depth, g.q[par][0], &g.cnt[it], ld_lazy->lazy, ld_lazy->new_list);
            hipLaunchKernelGGL(k_ld_contrib_list, dim3(lgrid), dim3(256), 0, g.stream, s->dev, ld.nvox[0], ld.nvox[1], ld.nvox[2], ld_lazy->lazy, ld_lazy->new_list, ld_lazy->func);
            hipLaunchKernelGGL(k_ld_build_list, dim3(lgrid), dim3(256), 0, g.stream, s->dev.n_lights, ld_lazy->lazy, ld_lazy->new_list, ld_lazy->func, ld_lazy->cdf, ld_lazy->func_int, ld_lazy->table);
            hipLaunchKernelGGL(k_ld_commit, dim3(1), dim3(1), 0, g.stream, ld_lazy->lazy);
        }
        if (s->has_textures) {
            const bool tex_sorted = bins_now && env_size("RSPT_TEXTURE_SORTED", 1) != 0;
            hipLaunchKernelGGL(s->has_quadrics ? k_texture_quad : s->has_spheres ? k_texture_sph : k_texture, dim3(sgrid), dim3(256), 0, g.stream, s->dev, s->tex, rd, P, g.q[par][0], &g.cnt[it].active,
                               tex_sorted ? g.q_sorted : (const uint32_t*)nullptr, tex_sorted ? &g.bin_info[it] : (const BinInfo*)nullptr);
        }
        hipLaunchKernelGGL((move && it >= move_first) ? shade_move_k : shade_k, dim3(hinted_grid(queue_hint, sgrid, 256)), dim3(256), sob_nd * sob_bits * sizeof(uint32_t), g.stream, s->dev, ld, rd, P, g.q[par][0], &g.cnt[it], &g.cnt[it + 1], g.q[par ^ 1][0],
                           g.q[par ^ 1][1], g.q[par ^ 1][2], counters ? g.totals + 2 : nullptr, sob_nd, sob_bits, (uint32_t)g.cap,
                           bins_now ? g.q_sorted : (const uint32_t*)nullptr, bins_now ? &g.bin_info[it] : (const BinInfo*)nullptr);
        ev_close(2, 0);
        it++;
        if (it < nominal_iters) continue;
        // after max_depth + 1 bounces only pending estimates and null-material passes remain
        if (max_iters == nominal_iters) break;
        if (((it - nominal_iters) & 7u) != 0 && it < max_iters) continue;  // look at the queue length every 8th iteration: an empty iteration costs three idle launches, a look costs a stream sync
        HIP_TRY(hipMemcpyAsync(g.look, &g.cnt[it], sizeof(QueueCounts), hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        const QueueCounts c = g.look[0];
        if (c.active == 0 && c.active_tail == 0) break;
        queue_hint = c.active + c.active_tail;
        if (it >= max_iters) {  // the reference's loop would still be running (path.rs:109-116 has no limit); these paths keep the radiance gathered so far
            truncated += c.active + c.active_tail;
            if (getenv("RSPT_VERBOSE") && c.active) {  // where the endless paths are: slot, film position and the ray in flight
                uint32_t slots[4];
                const uint32_t k = std::min(c.active, 4u);
                HIP_TRY(hipMemcpy(slots, g.q[it & 1][0], k * sizeof(uint32_t), hipMemcpyDeviceToHost));
                for (uint32_t j = 0; j < k; j++) {
                    rspt_ray r; float2 pf; float4 hc;
                    const PathBuf D = move ? move_pathbuf(it, move_first) : g.pb;   // (MOVE: queue entries are positions; the film position lives at the original slot)
                    uint32_t og = slots[j];
                    if (move && it > move_first) HIP_TRY(hipMemcpy(&og, D.orig + slots[j], sizeof og, hipMemcpyDeviceToHost));
                    HIP_TRY(hipMemcpy(&r, D.ray_cont + slots[j], sizeof r, hipMemcpyDeviceToHost));
                    HIP_TRY(hipMemcpy(&pf, D.p_film + og, sizeof pf, hipMemcpyDeviceToHost));
                    HIP_TRY(hipMemcpy(&hc, D.hit_cont + slots[j], sizeof hc, hipMemcpyDeviceToHost));
                    uint32_t o[3], dd[3], pr;
                    memcpy(o, r.o, 12); memcpy(dd, r.d, 12); memcpy(&pr, &hc.x, 4);
                    fprintf(stderr, "rspt: endless null-surface path: slot %u film (%.3f, %.3f) ray o %08x %08x %08x d %08x %08x %08x last prim %u\n",
                            slots[j], pf.x, pf.y, o[0], o[1], o[2], dd[0], dd[1], dd[2], pr);
                }
            }
            break;
        }
    }
    // MOVE: whatever is still queued (paths cut at max_iters; normally nothing) hands its radiance to the film's array
    if (move) hipLaunchKernelGGL(k_move_flush, dim3(grid_for(1)), dim3(256), 0, g.stream, move_pathbuf(it, move_first), g.q[it & 1][0], &g.cnt[it], (uint32_t)g.cap, it > move_first ? 1u : 0u);
    return RSPT_OK;
}
// ---- the batches of this shard: the pixel samplers in one go (render_tile_serial.h), the others batch by batch through their schedule above ----
int RenderRun::run() {
    int rc;
    if (pixel_sampler) {
        const size_t my_tiles = shard_tiles.size();
        const size_t min_tiles = env_size("RSPT_SERIAL_MIN_TILES", 2048);   // (round 4, statue frame under 02sequence, GPU vs 256 host threads, Msamples/s: 920 tiles 5.6 / 8.9, 2040: 11.2 / 8.0, 4080: 19.3 / 7.8, 8160: 26.7 / 7.3)
        if (!d->allow_slow_paths && my_tiles < min_tiles)
            return fail(RSPT_E_UNSUPPORTED, "a pixel sampler over %zu tiles: one lane per tile is slower than the host's tile loop below ~%zu tiles (set allow_slow_paths to run it anyway)", my_tiles, min_tiles);
    }
    if (pixel_sampler && (rc = run_tile_serial())) return rc;
    if (!pixel_sampler && (rc = film_index(g.pix_list, (uint32_t)n_pix))) return rc;
    for (size_t p0 = 0; !pixel_sampler && p0 < n_pix; p0 += pix_per_batch) {
        const uint32_t npx = (uint32_t)std::min(pix_per_batch, n_pix - p0);
        for (uint32_t s0 = (uint32_t)smp_begin; s0 < (uint32_t)smp_end; s0 += ns) {
            const uint32_t ns_b = std::min(ns, (uint32_t)smp_end - s0);  // Halton spp need not be a power of two
            Batch bt{(uint32_t)p0, npx, s0, ns_b, npx * ns_b};
            samples += bt.n;
            HIP_TRY(hipMemsetAsync(g.cnt, 0, (size_t)g.n_cnt * sizeof(QueueCounts), g.stream));
            if (shade_bins) HIP_TRY(hipMemsetAsync(g.bin_info, 0, (size_t)std::min<uint32_t>(g.n_bin_info, max_iters + 10) * sizeof(BinInfo), g.stream));
            // the path integrator's first shade launch knows what k_raygen would have written into L_eta / beta (PathBuf::fresh); RSPT_FRESH=0: written and read as before
            const bool fresh_ok = !volpath && !direct && !ao && env_size("RSPT_FRESH", 1) != 0;
            g.pb.fresh = fresh_ok ? 1u : 0u;
            if (realistic) hipLaunchKernelGGL(k_raygen_lens, dim3((bt.n + 255) / 256), dim3(256), 0, g.stream, rd, lens, bt, g.pb, g.pix_list, g.q[0][0], g.q[0][1], g.cnt);   // (path and ao only: validate)
            else
            hipLaunchKernelGGL(k_raygen, dim3((bt.n + 255) / 256), dim3(256), 0, g.stream, rd, bt, g.pb, g.pix_list, g.q[0][0], g.q[0][1], g.cnt);   // (MOVE or not: iteration 0 lives in set 0 = pb's own arrays, by slot)
            uint32_t it = 0;
            queue_hint = 0xffffffffu;
            if (volpath) rc = batch_volpath(bt, it);
            else if (direct) {
                rc = dl_lane ? batch_direct_lane(bt, it) : batch_direct(bt, it);
                if (rc == RSPT_DL_RETRY_LANE) {   // from here on the per-lane form serves this render; this batch starts over
                    dl_lane = true;
                    HIP_TRY(hipMemsetAsync(g.cnt, 0, (size_t)g.n_cnt * sizeof(QueueCounts), g.stream));
                    g.pb.fresh = 0u;
                    hipLaunchKernelGGL(k_raygen, dim3((bt.n + 255) / 256), dim3(256), 0, g.stream, rd, bt, g.pb, g.pix_list, g.q[0][0], g.q[0][1], g.cnt);
                    rc = batch_direct_lane(bt, it);
                }
            }
            else if (ao) rc = batch_ao(bt, it);
            else rc = batch_path(bt, it);
            if (rc) return rc;
            if (getenv("RSPT_QUEUE_LOG") && p0 == 0 && s0 == (uint32_t)smp_begin) {   // the queue lengths of the render's first batch, per wavefront iteration (profiles/rNN_shade_ledger.md)
                std::vector<QueueCounts> qc(it + 1);
                HIP_TRY(hipMemcpyAsync(qc.data(), g.cnt, (it + 1) * sizeof(QueueCounts), hipMemcpyDeviceToHost, g.stream));
                HIP_TRY(hipStreamSynchronize(g.stream));
                for (uint32_t k = 0; k <= it; k++)
                    fprintf(stderr, "rspt: queue it %u: active %u (+ %u that only wait for an estimate) closest %u any %u of %u paths\n", k, qc[k].active, qc[k].active_tail, qc[k].closest, qc[k].any, bt.n);
            }
            if (counters) hipLaunchKernelGGL(k_accum_counts, dim3(1), dim3(1), 0, g.stream, g.cnt, it, g.totals);
            film_stage(rd, bt, g.pb, g.pix_list);   // (MOVE: ended paths have written their radiance to pb.L_eta by original slot, move_pathbuf)
        }
    }
    queue_hint = 0xffffffffu;
    return RSPT_OK;
}
