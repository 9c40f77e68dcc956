// The pixel samplers' schedule: one lane per tile (tile_serial.h), over the state of render_run.h.  Host code of librspt.hip, included there once inside its anonymous namespace.
// k_tile_serial<INST, ALPHA, MODE> by [mode][inst][alpha].  Modes (tile_serial.h): 0 path, 1 ao, 2 volpath, 3 directlighting, 4 path with dynamic materials,
// 9 whitted; 5 - 8 and 10 = path / ao / volpath / directlighting / whitted with the instances' Transforms interpolated at the camera sample's time (round 6),
// which exist with INST only (tu_decl.h)
#define RSPT_TS_ROW(M) {{k_tile_serial<false, false, M>, k_tile_serial<false, true, M>}, {k_tile_serial<true, false, M>, k_tile_serial<true, true, M>}}
#define RSPT_TS_ROW_INST(M) {{nullptr, nullptr}, {k_tile_serial<true, false, M>, k_tile_serial<true, true, M>}}
typedef void (*TileKernel)(RSPT_TS_ARGS);
const TileKernel g_tile_serial[11][2][2] = {RSPT_TS_ROW(0), RSPT_TS_ROW(1), RSPT_TS_ROW(2), RSPT_TS_ROW(3), RSPT_TS_ROW(4), RSPT_TS_ROW_INST(5), RSPT_TS_ROW_INST(6), RSPT_TS_ROW_INST(7), RSPT_TS_ROW_INST(8), RSPT_TS_ROW(9), RSPT_TS_ROW_INST(10)};
#undef RSPT_TS_ROW_INST
#undef RSPT_TS_ROW
int RenderRun::run_tile_serial() {  // the pixel samplers: one lane per tile (tile_serial.h)
    int rc;

    // ---- one lane per tile (tile_serial.h) ----
    const int mode = s->has_animated ? (ao ? 6 : volpath ? 7 : whitted ? 10 : direct ? 8 : 5) : (ao ? 1 : volpath ? 2 : whitted ? 9 : direct ? 3 : s->has_dynamic ? 4 : 0);
    const TileKernel tile_k = g_tile_serial[mode][s->has_animated || s->has_instances][s->has_alpha];
    std::vector<TileRec> tiles;
    for (const auto& b : shard_tiles) {
        const int32_t x0 = sb[0] + (int32_t)b.first * ts, x1 = std::min(x0 + ts, sb[2]);
        const int32_t y0 = sb[1] + (int32_t)b.second * ts, y1 = std::min(y0 + ts, sb[3]);
        tiles.push_back(TileRec{(int16_t)x0, (int16_t)y0, (int16_t)x1, (int16_t)y1, (uint32_t)((int32_t)b.second * ntx + (int32_t)b.first), 0u, 0u});
    }
    const uint32_t n_tiles = (uint32_t)tiles.size();
    const uint32_t spp = (uint32_t)d->spp, nd = d->pixel_dimensions;
    // rows of every tile per pass: as many as the sample-result arrays (24 B per sample) allow
    const size_t samp_cap = std::max<size_t>(env_size("RSPT_SERIAL_SAMPLES", (size_t)1 << 28), (size_t)ts * spp);
    int32_t rows = ts;
    while (rows > 1 && (size_t)n_tiles * rows * ts * spp > samp_cap) rows--;
    if ((size_t)n_tiles * rows * ts * spp > ((size_t)1 << 31)) return fail(RSPT_E_UNSUPPORTED, "pixel sampler: %u tiles x %u spp do not fit one pass", n_tiles, spp);
    DevTemps guard;
    auto tmp = [&](auto** p, size_t n) { int r = dev_alloc(p, std::max<size_t>(n, 1)); if (!r) guard.p.push_back(*p); return r; };
    TileRec* tiles_d = nullptr; float4* samp_L = nullptr; float2* samp_pf = nullptr; float* a1 = nullptr; float2* a2 = nullptr; uint64_t* rng_state = nullptr; uint64_t* rng_saved = nullptr;
    // the integrator's 2-D sample arrays (request_2d_array in preprocess): ao one of n_samples (ao.rs:47-49); directlighting, strategy all,
    // two per light and recursion level (directlighting.rs:54-70)
    float2* arr = nullptr; uint32_t* arr_sz_d = nullptr; uint32_t* arr_base_d = nullptr; int32_t* nls_d = nullptr;
    std::vector<uint32_t> arr_sz;
    if (ao) arr_sz.push_back(d->ao_n_samples);
    if (direct && !whitted && d->direct_strategy == RSPT_DIRECT_SAMPLE_ALL)   // (whitted.rs requests no arrays)
        for (uint32_t lvl = 0; lvl < d->max_depth; lvl++)
            for (uint32_t j = 0; j < s->dev.n_lights; j++) { const uint32_t n = d->n_light_samples ? (uint32_t)d->n_light_samples[j] : 1u; arr_sz.push_back(n); arr_sz.push_back(n); }
    std::vector<uint32_t> arr_base(arr_sz.size());
    uint32_t arr_total = 0;
    for (size_t a = 0; a < arr_sz.size(); a++) { arr_base[a] = arr_total * spp; arr_total += arr_sz[a]; }
    if ((size_t)arr_total * spp * n_tiles > ((size_t)1 << 31)) return fail(RSPT_E_UNSUPPORTED, "pixel sampler: %u sample-array points x %u spp x %u tiles", arr_total, spp, n_tiles);
    if (!arr_sz.empty()) {
        if ((rc = tmp(&arr, (size_t)arr_total * spp * n_tiles)) || (rc = tmp(&arr_sz_d, arr_sz.size())) || (rc = tmp(&arr_base_d, arr_sz.size()))) return rc;
        HIP_TRY(hipMemcpyAsync(arr_sz_d, arr_sz.data(), arr_sz.size() * 4, hipMemcpyHostToDevice, g.stream));
        HIP_TRY(hipMemcpyAsync(arr_base_d, arr_base.data(), arr_base.size() * 4, hipMemcpyHostToDevice, g.stream));
    }
    if (direct && d->n_light_samples && s->dev.n_lights) {
        if ((rc = tmp(&nls_d, s->dev.n_lights))) return rc;
        HIP_TRY(hipMemcpyAsync(nls_d, d->n_light_samples, s->dev.n_lights * sizeof(int32_t), hipMemcpyHostToDevice, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));   // (the caller's array, and the vectors above, must outlive the copies)
    }
    uint32_t* c_pixel_d = nullptr; uint32_t* trunc_d = nullptr; uint32_t* pass_pix = nullptr;
    const size_t max_samples = (size_t)n_tiles * rows * ts * spp;
    if ((rc = tmp(&tiles_d, n_tiles)) || (rc = tmp(&samp_L, max_samples)) || (rc = tmp(&samp_pf, max_samples)) || (rc = tmp(&a1, (size_t)nd * spp * n_tiles)) ||
        (rc = tmp(&a2, (size_t)nd * spp * n_tiles)) || (rc = tmp(&rng_state, 2 * (size_t)n_tiles)) || (rc = tmp(&rng_saved, ld.lazy ? 2 * (size_t)n_tiles : 1)) || (rc = tmp(&c_pixel_d, 32)) || (rc = tmp(&trunc_d, 2)) ||
        (rc = tmp(&pass_pix, (size_t)n_tiles * rows * ts)))
        return rc;
    HIP_TRY(hipMemsetAsync(trunc_d, 0, sizeof(uint32_t), g.stream));
    if (d->sampler_kind == RSPT_SAMPLER_MAXMINDIST) HIP_TRY(hipMemcpyAsync(c_pixel_d, d->maxmin_c_pixel, 32 * sizeof(uint32_t), hipMemcpyHostToDevice, g.stream));
    const PixDesc pd{d->sampler_kind, spp, d->sampler_kind == RSPT_SAMPLER_RANDOM ? 0u : nd, d->strat_x, d->strat_y, d->strat_jitter, c_pixel_d, a1, a2, rng_state, arr, arr_sz_d, arr_base_d, (uint32_t)arr_sz.size(), arr_total, d->ao_cos_sample, nls_d, d->direct_strategy, dl_tex, dl_tex_rows, dl_dyn};
    // lanes per wave: a lane that shares its wave waits whenever the others diverge (measured: four lanes of a wave take four times one lane's
    // time — no overlap at all), so the tiles are spread over waves, up to twice what the chip holds at these kernels' 2 waves / SIMD
    // (256 CUs x 4 SIMDs x 2 = 2048) before doubling up: C3 frame, 8160 tiles, 02sequence — 2048: 21.9, 4096: 24.7, 8192: 21.7 Msamples/s;
    // builds forced to 3 / 4 waves per SIMD (168 / 128 VGPRs, 2.3 / 2.5 KB of scratch) lose to the spills: 17.8 - 21.5
    uint32_t lanes = 1;
    while (lanes < 64 && (n_tiles + lanes - 1) / lanes > (uint32_t)env_size("RSPT_SERIAL_WAVES", 4096)) lanes *= 2;
    if (s->has_dynamic && (rc = ensure_dyn_built(((n_tiles + lanes - 1) / lanes) * 64u))) return rc;   // one lobe record per thread of the launch
    PathBuf fpb = g.pb;
    fpb.L_eta = samp_L; fpb.p_film = samp_pf;
    const uint32_t serial_iters = nominal_iters + 1u + (s->has_null_material ? (uint32_t)env_size("RSPT_NULL_PASSES", 1024) : 0u);
    std::vector<uint32_t> pl;
    for (int32_t r0 = 0; r0 < ts; r0 += rows) {
        const int32_t r1 = std::min(r0 + rows, ts);
        pl.clear();
        for (TileRec& t : tiles) {
            t.pix0 = (uint32_t)pl.size();
            for (int32_t y = t.y0 + r0; y < t.y0 + r1 && y < t.y1; y++)
                for (int32_t x = t.x0; x < t.x1; x++) pl.push_back(((uint32_t)(uint16_t)(int16_t)y << 16) | (uint32_t)(uint16_t)(int16_t)x);
        }
        if (pl.empty()) continue;
        HIP_TRY(hipStreamSynchronize(g.stream));  // the previous pass still reads tiles_d / pass_pix
        HIP_TRY(hipMemcpyAsync(tiles_d, tiles.data(), n_tiles * sizeof(TileRec), hipMemcpyHostToDevice, g.stream));
        HIP_TRY(hipMemcpyAsync(pass_pix, pl.data(), pl.size() * sizeof(uint32_t), hipMemcpyHostToDevice, g.stream));
        const dim3 grid((n_tiles + lanes - 1) / lanes);
        // on-demand light voxels: a lane claims the voxels it finds without a row (dev_scene.h light_row_try) and goes on with row 0; the claimed rows are
        // built and the rows of the tiles rendered again from the saved generator states, until a run claims nothing — only that run's samples are kept
        // (a wrong row can change how many dimensions an estimate draws, so a run may leave the true paths after its first missing voxel: each
        // round completes at least the first one along every true chain)
        if (ld.lazy) {
            HIP_TRY(hipMemcpyAsync(rng_saved, rng_state, 2 * (size_t)n_tiles * sizeof(uint64_t), hipMemcpyDeviceToDevice, g.stream));
            HIP_TRY(hipMemcpyAsync(trunc_d + 1, trunc_d, sizeof(uint32_t), hipMemcpyDeviceToDevice, g.stream));
        }
        for (uint32_t lazy_round = 0;; lazy_round++) {
        if (ld.lazy && lazy_round > 0) {
            HIP_TRY(hipMemcpyAsync(rng_state, rng_saved, 2 * (size_t)n_tiles * sizeof(uint64_t), hipMemcpyDeviceToDevice, g.stream));
            HIP_TRY(hipMemcpyAsync(trunc_d, trunc_d + 1, sizeof(uint32_t), hipMemcpyDeviceToDevice, g.stream));
        }
        ev_open(2, 0);
        hipLaunchKernelGGL(tile_k, grid, dim3(64), 0, g.stream, s->dev, s->tex, ld, rd, g.pb, pd, tiles_d, n_tiles, lanes, r0, r1, samp_L, samp_pf, serial_iters, trunc_d);
        ev_close(2, 0);
        if (!ld.lazy) break;
        uint32_t claimed = 0;
        if ((rc = build_claimed_rows(&claimed))) return rc;
        if (claimed == 0) break;
        if (lazy_round > 64) return fail(RSPT_E_UNSUPPORTED, "pixel sampler: on-demand light voxels did not settle in 64 rounds (not a device fault: the caller keeps its CPU loop, or asks for the eager table)");
        }
        const uint32_t npx = (uint32_t)pl.size();
        Batch bt{0u, npx, 0u, spp, npx * spp};
        samples += bt.n;
        if ((rc = film_index(pass_pix, npx))) return rc;
        film_stage(rd, bt, fpb, pass_pix);
    }
    uint32_t tv = 0;
    HIP_TRY(hipMemcpyAsync(&tv, trunc_d, sizeof tv, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    truncated += tv;
    return RSPT_OK;
}
