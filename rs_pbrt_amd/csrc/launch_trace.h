// One launch of the traversal stage: the descriptor a caller fills (TraceCall), the kernel choice per scene and switch, and the shade stage's
// instantiations.  Host code of librspt.hip, included there once inside its anonymous namespace (it uses that file's Ctx g and allocators).
// upper bound of the queue lengths of the launches that follow, when the host knows one (the null-surface tail of a render looks at
// its queue every 8th iteration and the queues only shrink): a few hundred paths do not need 1280 persistent workgroups each copying
// the root-side records into LDS
uint32_t hinted_grid(uint32_t hint, uint32_t full, uint32_t per_block) {
    if (hint == 0xffffffffu) return full;
    const uint64_t need = (2ull * hint + per_block - 1) / per_block + 1;
    return (uint32_t)std::min<uint64_t>(full, need);
}
// does the production trace kernel ever hand rays to k_trace_fixup?  Not the four-box kernel with all its spill rows (RSPT_W4_MAX_STACK)
bool trace_can_overflow(const rspt_scene_s* s) {
    const size_t which = env_size("RSPT_TRACE_KERNEL", 2);
    const size_t rows = std::min<size_t>(env_size("RSPT_W4_SPILL_ROWS", RSPT_W4_SPILL), RSPT_W4_SPILL);
    return s->has_instances || (s->has_alpha && !s->w4_ok) || !(which >= 2 && s->w4_ok) || RSPT_W4_LDS + rows < RSPT_W4_MAX_STACK;  // (two stacked aggregates + leaf continuations can pass the bound)
}
uint32_t trace_grid() { return grid_for((uint32_t)env_size("RSPT_TRACE_BLOCKS_PER_CU", 5)); }
// One launch of the traversal stage.  Kernel choice: scenes with object instances or alpha-masked meshes take the <INST, ALPHA>
// instantiations (template flags, so that the plain kernels stay the ones measured in DESIGN.md); counters and RSPT_TRACE_KERNEL=0
// use the reference-order loop; a scene whose records outgrow the four-box reference fields stays on the two-box kernel.
#ifndef RSPT_PW_CHUNK_CAMERA_DEFAULT
#define RSPT_PW_CHUNK_CAMERA_DEFAULT 1024   // measured on the C3 stand-in, same box, alternating: 256 -> 2025 / 2029, 1024 -> 2075 / 2070, 4096 -> 2024 / 2030, 16384 -> 1900 Msamples/s
                                            // (C2: 473.9 / 473.3 / 471.1 at 256 / 1024 / 4096); the incoherent launches keep 256 (512: C3 2061 with the camera launch at 1024)
#endif
#ifndef RSPT_PW_REFILL_CAMERA_DEFAULT
#define RSPT_PW_REFILL_CAMERA_DEFAULT 48   // a wave of coherent camera rays refills when three quarters of its lanes are idle (the incoherent launches: RSPT_PW_REFILL = 16)
#endif
#ifndef RSPT_PW_ENTER
#define RSPT_PW_ENTER 24   // C5 stand-in, every instance moving (profiles/r06_c5_enter_sweep.txt): 1 -> 142, 8 -> 170, 16 -> 182, 24 -> 183, 32 -> 180 Msamples/s
#endif
#ifndef RSPT_PW_LEAF_ANY_Q_DEFAULT
#define RSPT_PW_LEAF_ANY_Q_DEFAULT 16   // parked lanes that start a leaf phase of k_trace_w4q (trace_w4q.h).  C2 frame, one box, one process (profiles/shadow_defer_ab.txt section 6):
                                        // 8 -> 554.9 / 553.4 / 554.7 / 554.4, 16 -> 561.6 / 561.3, 24 -> 561.9, 32 -> 556.6 / 556.8, 48 -> 527.3 Msamples/s; the C3 stand-in does not resolve 8 / 16 / 32
#endif
// What one trace launch reads and writes. Every field defaults to "absent": a call site names what it uses.
struct TraceCall {
    const uint32_t* queue = nullptr; const uint32_t* count_ptr = nullptr; uint32_t count_imm = 0;   // the queue entries to trace; their number on the device, or known to the host
    uint32_t* cursor = nullptr;                                  // the persistent kernels' fetch cursor (QueueCounts: the overflow word sits two after it)
    const rspt_ray* ra = nullptr; const rspt_ray* rb = nullptr;  // rays / outputs of the entries without / with the MIS flag
    float4* oa = nullptr; float4* ob = nullptr;
    uint32_t* occ = nullptr;                                     // any hit: the occlusion flags
    rspt_hit* hits = nullptr;                                    // OUT_MODE 1 (the trace hook): full hit records
    unsigned long long* counters = nullptr; uint32_t* xcd_cursors = nullptr;   // the node / triangle counters; eight zeroed words: XCD-affine dealing where RSPT_XCD_DEAL asks for it
    int lane = 0;                      // 0 = the library's main stream; 1 = the second stream with its own overflow list and spill rows
    bool count = false;                // the reference-order kernel with its node / triangle counters
    bool camera_launch = false;        // the camera rays of a batch (a pixel-major queue): RSPT_PW_CHUNK_CAMERA / _REFILL_CAMERA / _LEAF_CAMERA
    int force_any_q = -1;              // tune_any's measurement of the two shadow-ray kernels: 0 / 1 forces the plain / the quantised one
    int force_camera_pk = -1;          // tune_camera's measurement of the camera-ray kernels: 0 / 1 / 2 / 3 / 4 forces k_trace_w4 / the packet kernel / the frustum packet kernel / its bundles of two / of four packets
    uint32_t* inst_out = nullptr;      // where a closest-hit launch records the instance of each hit instead of g.hit_inst (volpath's shadow-ray segments)
    uint32_t queue_hint = 0xffffffffu; // upper bound of the queue's length when the host knows one (hinted_grid), 0xffffffff: none
};
// what every persistent-wave launch needs besides its kernel: the lane's stream with its overflow list and spill rows, the hinted grid, the refill / leaf-phase
// thresholds and the claim size.  `camera`: the camera-ray launch's own values; the sphere kernels never take them
struct TracePre { hipStream_t stream; uint32_t* ovf; uint2* spill; uint32_t pgrid; int refill, leaf; uint32_t chunk; };
TracePre trace_pre(const TraceCall& c, bool camera) {
    TracePre p; p.stream = c.lane ? g.stream2 : g.stream;
    p.ovf = g.ovf + (c.lane ? 2 * g.ovf_cap / 3 : 0);
    p.spill = g.spill + (c.lane ? g.spill_threads * RSPT_W4_SPILL : 0);
    p.pgrid = hinted_grid(c.queue_hint, pw_grid(), RSPT_PW_BLOCK);
    // rays a wave claims per global atomic: 256 for the incoherent launches; the camera-ray launch of a batch (pixel-major queue: a chunk is a run of samples of one pixel
    // or its neighbours) takes RSPT_PW_CHUNK_CAMERA (TraceCall::camera_launch, set by the path integrator's loop)
    // refill / leaf-phase thresholds; the camera-ray launch may take its own (RSPT_PW_REFILL_CAMERA / RSPT_PW_LEAF_CAMERA: coherent rays reach their leaves together)
    // (camera launch, C3 stand-in, one box, alternating: refill 16 -> 2079 / 2067 Msamples/s, 32 -> 2083 / 2083, 48 -> 2114 / 2113, 64 -> 2105 / 2101; leaf 16 / 24 / 32 at refill 16: 2061 / 2059 / 2046)
    p.refill = (int)(camera ? env_size("RSPT_PW_REFILL_CAMERA", RSPT_PW_REFILL_CAMERA_DEFAULT) : env_size("RSPT_PW_REFILL", RSPT_PW_REFILL));
    p.leaf = (int)(camera ? env_size("RSPT_PW_LEAF_CAMERA", env_size("RSPT_PW_LEAF", RSPT_PW_LEAF)) : env_size("RSPT_PW_LEAF", RSPT_PW_LEAF));
    p.chunk = (uint32_t)std::min<size_t>(std::max<size_t>((camera ? env_size("RSPT_PW_CHUNK_CAMERA", RSPT_PW_CHUNK_CAMERA_DEFAULT) : env_size("RSPT_PW_CHUNK", RSPT_PW_CHUNK)) & ~(size_t)63, 64), 1u << 20);
    return p;
}
// can the packet kernel (trace_packet.h) serve a closest-hit launch of this scene?  Plain triangle scenes on the four-box records with the leaves' own boxes at hand (the
// array built for k_trace_w4q), an interior root, the default workgroup shape, one fetch cursor
bool camera_packet_ok(const rspt_scene_s* s, size_t which, const uint32_t* xcur) {
    return which >= 2 && s->w4_ok && s->w4 && s->leaf_boxes && !s->has_instances && !s->has_alpha && !s->has_spheres && !(s->w4_root & RSPT_REF_LEAF) &&
           env_size("RSPT_W4_SHAPE", RSPT_W4_SHAPE_DEFAULT) == 0 && !xcur;
}
// which kernel a closest-hit launch asks for: 0 = k_trace_w4, 1 = k_trace_w4pk (trace_packet.h), 2 = k_trace_w4pf (trace_frustum.h), 3 / 4 = k_trace_w4pb with bundles of
// two / four packets (trace_bundle.h)
int camera_packet_wanted(const rspt_scene_s* s, const TraceCall& c) {
    int v;
    const char* e = getenv("RSPT_CAMERA_PACKET");
    if (c.force_camera_pk >= 0) v = c.force_camera_pk;
    else if (e && *e) v = atoi(e);
    else v = c.camera_launch ? s->camera_pk_choice : 0;
    return v <= 0 ? 0 : (v >= 2 && v <= 4 ? v : 1);
}
// workgroups per CU of a bundle kernel: what its registers allow (a workgroup is one wave per SIMD), asked of the runtime once per instantiation
template <int OUT_MODE, int R>
uint32_t bundle_blocks_per_cu() {
    static int blocks = 0;
    if (blocks == 0) {
        int b = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, reinterpret_cast<const void*>(k_trace_w4pb<OUT_MODE, R>), RSPT_PW_BLOCK, 0) != hipSuccess) { (void)hipGetLastError(); b = 0; }
        blocks = std::min(std::max(b, 1), 8);
    }
    return (uint32_t)blocks;
}
// One launch of a four-box kernel (k_trace_w4 / k_trace_w4quad: RSPT_W4_ARGS), of a packet kernel (RSPT_PK_ARGS) and of k_trace_fixup (RSPT_FIXUP_ARGS): a call
// site names what differs between the sites, the rest is the call's and its TracePre's.  (QueueCounts layout: the overflow word sits two after its cursor)
template <typename K>
void launch_w4(K kern, uint32_t grid, uint32_t block, size_t lds, const rspt_scene_s* s, const TraceCall& c, const TracePre& p, int leaf, uint32_t spill_rows, uint32_t* hi, uint32_t* xcur,
               uint32_t chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, p.stream, s->dev, s->tex, s->w4, s->big_leaves, s->w4_root, c.queue, c.count_ptr, c.count_imm, c.cursor, c.ra, c.rb, c.oa, c.ob, c.occ,
                       c.hits, c.cursor + 2, p.ovf, p.spill, spill_rows, p.refill, leaf, s->w4_top, hi, xcur, chunk);
}
template <typename K>
void launch_pk(K kern, uint32_t grid, const rspt_scene_s* s, const TraceCall& c, const TracePre& p, uint32_t chunk) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(RSPT_PW_BLOCK), 0, p.stream, s->dev, s->w4, s->big_leaves, s->w4_root, c.queue, c.count_ptr, c.count_imm, c.cursor, c.ra, c.rb, c.oa, c.ob, c.hits,
                       chunk, s->leaf_boxes);
}
template <typename K>
void launch_fixup(K kern, uint32_t grid, const rspt_scene_s* s, const TraceCall& c, const TracePre& p, uint32_t* hi) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(RSPT_TRACE_BLOCK), 0, p.stream, s->dev, s->tex, c.cursor + 2, p.ovf, c.ra, c.rb, c.oa, c.ob, c.occ, c.hits, hi);
}
template <bool ANY, int OUT_MODE, bool INST, bool ALPHA>
void launch_trace_v(uint32_t grid, const rspt_scene_s* s, const TraceCall& c, uint32_t* xcur) {
    const SceneDev& sc = s->dev;
    // RSPT_TRACE_KERNEL: 0 = k_trace (reference-order single-ray loop), 1 = k_trace_pw (persistent waves, two boxes
    // per record), 2 = k_trace_w4 (persistent waves, four boxes per record; default).
    // (A quad-per-ray variant with one coalesced 64-byte fetch per step was measured 35 % slower: the
    //  replicated control flow made it VALU-bound with 16 rays per wave)
    const size_t which = env_size("RSPT_TRACE_KERNEL", 2);
    const TracePre p = trace_pre(c, c.camera_launch);
    uint32_t* hi = (INST && OUT_MODE == 0 && !ANY) ? (c.inst_out ? c.inst_out : g.hit_inst) : nullptr;
    const bool special = INST || ALPHA;
    // moving instances: k_trace_w4<.., INST, 0, ANIM> (round 5; RSPT_ANIM_W4=0: the reference-order loop with the interpolation, as before)
    const bool anim_w4 = s->has_animated && s->w4_ok && which >= 2 && env_size("RSPT_ANIM_W4", 1) != 0 && env_size("RSPT_INSTANCE_KERNEL", 1) != 0;   // (round 6: the reference-order loop serves moving instances next to masks too, so every A/B switch stays bit-exact)
    const bool slow = c.count || which == 0 || (s->has_animated && !anim_w4) || (special && (!s->w4_ok || env_size("RSPT_INSTANCE_KERNEL", 1) == 0));
    if (slow) {
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(RSPT_TRACE_BLOCK), 0, p.stream, sc, s->tex, c.queue, c.count_ptr, c.count_imm, c.ra, c.rb, c.oa, c.ob, c.occ, c.hits, c.counters, hi);
        };
        if (INST && s->has_animated)   // moving instances (alone or next to alpha-masked meshes): the reference-order loop with the interpolation (its own instantiations; no node / triangle counters)
            go(k_trace<ANY, OUT_MODE, false, true, ALPHA, true>);
        else if (c.count)
            go(k_trace<ANY, OUT_MODE, true, INST, ALPHA>);
        else
            go(k_trace<ANY, OUT_MODE, false, INST, ALPHA>);
        return;
    }
    const uint32_t pw_chunk = p.chunk | (env_size("RSPT_PW_ADAPT", 1) != 0 ? 0u : 1u);   // (bit 0: the kernels do not shrink the claim on short queues — trace_w4.h)
    grid = hinted_grid(c.queue_hint, grid, RSPT_TRACE_BLOCK);
    uint32_t* n_overflow = c.cursor + 2;  // QueueCounts layout: overflow word sits two after its cursor
    const uint32_t spill_rows = (uint32_t)std::min<size_t>(env_size("RSPT_W4_SPILL_ROWS", RSPT_W4_SPILL), RSPT_W4_SPILL);
    if constexpr (INST) {
        if (anim_w4) {   // moving instances; next to alpha-masked meshes the masks in line (ALPHA = 2) where every mask allows it, else through alpha_pass
            // RSPT_PW_ENTER: lanes in front of an instance wait until that many of a wave do (trace_w4.h, the entry phase); it rides in bits 8.. of the leaf threshold
            const int pw_enter = (int)std::min<size_t>(std::max<size_t>(env_size("RSPT_PW_ENTER", RSPT_PW_ENTER), 1), 64);
            auto go = [&](auto kern) { launch_w4(kern, p.pgrid, RSPT_PW_BLOCK, 0, s, c, p, (p.leaf & 0xff) | (pw_enter << 8), spill_rows, hi, xcur, pw_chunk); };
            if constexpr (ALPHA) { if (s->alpha_simple) go(k_trace_w4<ANY, OUT_MODE, true, 2, true>); else go(k_trace_w4<ANY, OUT_MODE, true, 1, true>); }
            else go(k_trace_w4<ANY, OUT_MODE, true, 0, true>);
            launch_fixup(k_trace_fixup<ANY, OUT_MODE, true, ALPHA, true>, grid, s, c, p, hi);
            return;
        }
    }
    if constexpr (ANY && !INST && !ALPHA) {
        // round 6: shadow rays of plain scenes walk the 64-byte quantised records (trace_w4q.h; RSPT_ANY_Q=0: the plain kernel).  Occlusion flags byte-identical.
        // Which of the two is faster depends on the rays, not on the scene's size: the quantised records win where the plain kernel is bound by L1 lane requests (C2's incoherent
        // shadow rays through a dense soup: +6 % on the frame) and lose where it is bound by VALU issue with half its fetches in LDS (the C3 stand-in's coherent ones: -2.5 %;
        // profiles/r06_any_q_ab.txt).  RSPT_ANY_Q=0 / 1 forces one; otherwise the scene's measured choice (rspt_scene_s::any_q_choice), the plain kernel until it exists.
        const char* q_env = getenv("RSPT_ANY_Q");
        const bool use_q = c.force_any_q >= 0 ? c.force_any_q != 0 : (q_env && *q_env ? atoi(q_env) != 0 : s->any_q_choice > 0);
        if (use_q && which >= 2 && s->w4q && !(s->w4_root & RSPT_REF_LEAF) && c.ra == c.rb && env_size("RSPT_W4_SHAPE", RSPT_W4_SHAPE_DEFAULT) == 0 && !xcur && spill_rows == RSPT_W4_SPILL) {
            // the leaf-phase threshold of this kernel is its own (RSPT_PW_LEAF_ANY_Q): its leaf phase is the any-hit one (no t_max to hand back to the node steps), so
            // parked lanes can wait for a fuller phase than the closest-hit kernels' RSPT_PW_LEAF = 8 allows — RSPT_PW_LEAF_ANY_Q_DEFAULT above
            const int q_leaf = (int)std::min<size_t>(std::max<size_t>(env_size("RSPT_PW_LEAF_ANY_Q", RSPT_PW_LEAF_ANY_Q_DEFAULT), 1), 64);
            hipLaunchKernelGGL((k_trace_w4q<OUT_MODE>), dim3(p.pgrid), dim3(RSPT_PW_BLOCK), 0, p.stream, sc, s->w4q, s->big_leaves, s->w4_root, c.queue, c.count_ptr, c.count_imm, c.cursor,
                               c.ra, c.occ, c.hits, reinterpret_cast<uint32_t*>(p.spill), p.refill, q_leaf, s->w4_top,
                               pw_chunk | (env_size("RSPT_ANY_Q_LATE", 1) != 0 ? 2u : 0u) /* bit 1: the exact leaf-box test only behind a triangle hit (trace_w4q.h) */, s->leaf_boxes);
            return;
        }
    }
    if constexpr (!ANY && !INST && !ALPHA) {
        // The camera rays of a batch (a pixel-major queue: the 64 lanes of a wave hold samples of one pixel) walk the tree as 64-ray packets (trace_packet.h): records and
        // triangles fetched once per wave, one stack per wave.  Hit records byte-identical.  RSPT_CAMERA_PACKET=0 / 1 / 2 / 3 / 4 forces the old / the packet / the frustum packet kernel / its bundle forms — 1 to 4 for EVERY
        // closest-hit launch that qualifies, the trace hook included (incoherent rays are slow there, and right); otherwise the scene's measured choice
        // (rspt_scene_s::camera_pk_choice) serves the camera launches, k_trace_w4 until it exists.
        const int pk = camera_packet_wanted(s, c);
        if (pk >= 3 && camera_packet_ok(s, which, xcur)) {
            // RSPT_CAMERA_PACKET=3 / 4: the frustum walk once per bundle of two / four packets (trace_bundle.h: with 128 / 256 or more samples per pixel a bundle is one pixel), same
            // arguments, same records; the grid is what the kernel's registers allow
            auto go = [&](auto kern, uint32_t per_cu) { launch_pk(kern, hinted_grid(c.queue_hint, grid_for(per_cu), RSPT_PW_BLOCK), s, c, p, pw_chunk); };
            if (pk == 3) go(k_trace_w4pb<OUT_MODE, 2>, bundle_blocks_per_cu<OUT_MODE, 2>());
            else go(k_trace_w4pb<OUT_MODE, 4>, bundle_blocks_per_cu<OUT_MODE, 4>());
            return;
        }
        if (pk && camera_packet_ok(s, which, xcur)) {
            // (no spill rows and 6 KB of LDS: its grid is its own — six workgroups per CU = the six waves per SIMD its 79 VGPRs allow; RSPT_PK_BLOCKS_PER_CU for A/B builds)
            const uint32_t kgrid = hinted_grid(c.queue_hint, grid_for((uint32_t)std::min<size_t>(std::max<size_t>(env_size("RSPT_PK_BLOCKS_PER_CU", 6), 1), 8)), RSPT_PW_BLOCK);
            // RSPT_CAMERA_PACKET=2: the packet walk with one frustum test per record instead of the per-ray slot tests (trace_frustum.h), same arguments, same records
            launch_pk(pk == 2 ? k_trace_w4pf<OUT_MODE> : k_trace_w4pk<OUT_MODE>, kgrid, s, c, p, pw_chunk);
            return;
        }
    }
    if constexpr (!INST && !ALPHA) {
        // RSPT_W4_SHAPE: 0 = five 256-thread workgroups per CU, 56 root-side records in LDS each; 1 = ONE 1024-thread workgroup per CU with 512 records;
        // 2 = two 512-thread workgroups with 256 records each (trace_w4.h BLOCK / TOPCAP; dynamic LDS, 152 KB per CU either way)
        const size_t shape = which >= 2 && s->w4_ok ? env_size("RSPT_W4_SHAPE", RSPT_W4_SHAPE_DEFAULT) : 0;
        if (shape == 1 || shape == 2) {
            auto go = [&](auto kern, uint32_t block, uint32_t topcap, uint32_t per_cu) -> bool {
                const size_t lds = (size_t)8 * RSPT_W4_LDS * block + (size_t)112 * topcap;
                static bool attr_set[2][2][2][3] = {};
                bool& done = attr_set[ANY ? 1 : 0][OUT_MODE ? 1 : 0][0][shape];
                static bool attr_bad[2][2][2][3] = {};
                bool& bad = attr_bad[ANY ? 1 : 0][OUT_MODE ? 1 : 0][0][shape];
                if (!done) { bad = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess; (void)hipGetLastError(); done = true; }
                if (bad) return false;   // the device refuses that much dynamic LDS: the default shape serves the launch
                const uint32_t bgrid = hinted_grid(c.queue_hint, grid_for(per_cu), block);
                launch_w4(kern, bgrid, block, lds, s, c, p, p.leaf, spill_rows, hi, xcur, pw_chunk);
                return true;
            };
            const bool launched = shape == 1 ? go(k_trace_w4<ANY, OUT_MODE, false, 0, false, 1024, 512>, 1024u, 512u, 1u) : go(k_trace_w4<ANY, OUT_MODE, false, 0, false, 512, 256>, 512u, 256u, 2u);
            if (launched) {
                if (trace_can_overflow(s)) launch_fixup(k_trace_fixup<ANY, OUT_MODE, INST, ALPHA>, grid, s, c, p, hi);
                return;
            }
        }
    }
    if (ALPHA && s->alpha_simple)   // every mask of the scene is evaluated in line (kernels.h alpha_simple): the traversal keeps its register budget
        launch_w4(k_trace_w4<ANY, OUT_MODE, INST, ALPHA ? 2 : 0>, p.pgrid, RSPT_PW_BLOCK, 0, s, c, p, p.leaf, spill_rows, hi, xcur, pw_chunk);
    else if (special || (which >= 2 && s->w4_ok))
        launch_w4(k_trace_w4<ANY, OUT_MODE, INST, ALPHA ? 1 : 0>, p.pgrid, RSPT_PW_BLOCK, 0, s, c, p, p.leaf, spill_rows, hi, xcur, pw_chunk);
    else
        hipLaunchKernelGGL((k_trace_pw<ANY, OUT_MODE>), dim3(p.pgrid), dim3(RSPT_PW_BLOCK), 0, p.stream, sc, s->pairs, c.queue, c.count_ptr, c.count_imm, c.cursor, c.ra, c.rb, c.oa, c.ob, c.occ, c.hits, n_overflow, p.ovf,
                           p.refill, p.leaf);
    // with every spill row in use the plain four-box kernel cannot overflow (RSPT_W4_MAX_STACK): no second pass to launch
    if (trace_can_overflow(s)) launch_fixup(k_trace_fixup<ANY, OUT_MODE, INST, ALPHA>, grid, s, c, p, hi);
}
// Scenes with spheres (ABI 23): k_trace_w4<.., SPH = true> with every spill row (a non-instanced four-box walk cannot then overflow, so no
// k_trace_fixup — whose reference-order loop has no sphere test); no node counters, no quantised shadow-ray records (k_trace_w4q walks triangle
// leaves only, and tune_any never measures them), no big-workgroup shapes: RSPT_COUNTERS, RSPT_TRACE_KERNEL, RSPT_ANY_Q, RSPT_W4_SHAPE and
// RSPT_W4_SPILL_ROWS do not apply.  OUT_MODE 1 is the trace hook (main stream); OUT_MODE 0 the render's queues, on the stream the caller's lane
// names with that lane's overflow list and spill rows (the two-stream shadow-ray overlap, RSPT_TRACE_STREAMS).  rspt_trace_device and
// rspt_render check w4_ok first; rspt_render refuses RSPT_COUNTERS on sphere scenes.
template <bool ANY, int OUT_MODE>
void launch_trace_sph(const rspt_scene_s* s, const TraceCall& c, uint32_t* xcur) {
    const TracePre p = trace_pre(c, false);
    auto go = [&](auto kern) { launch_w4(kern, p.pgrid, RSPT_PW_BLOCK, 0, s, c, p, p.leaf, (uint32_t)RSPT_W4_SPILL, nullptr, xcur, p.chunk); };
    if (s->has_quadrics) {   // ABI 27: a disk or a cylinder in the scene: the kernels whose leaf phase reads the slot's kind (trace_w4.h k_trace_w4quad)
        if (OUT_MODE == 1 && getenv("RSPT_VERBOSE"))   // (the trace hook only: a render launches this hundreds of times)
            fprintf(stderr, "rspt: trace instantiation 'k_trace_w4quad<%s, alpha %d>'\n", ANY ? "any" : "closest", !s->has_alpha ? 0 : (s->alpha_simple ? 2 : 1));
        if (!s->has_alpha) go(k_trace_w4quad<ANY, OUT_MODE, 0>);
        else if (s->alpha_simple) go(k_trace_w4quad<ANY, OUT_MODE, 2>);
        else go(k_trace_w4quad<ANY, OUT_MODE, 1>);
        return;
    }
    if (!s->has_alpha) go(k_trace_w4<ANY, OUT_MODE, false, 0, false, RSPT_PW_BLOCK, RSPT_W4_TOP, true>);
    else if (s->alpha_simple) go(k_trace_w4<ANY, OUT_MODE, false, 2, false, RSPT_PW_BLOCK, RSPT_W4_TOP, true>);
    else go(k_trace_w4<ANY, OUT_MODE, false, 1, false, RSPT_PW_BLOCK, RSPT_W4_TOP, true>);
}
template <bool ANY, int OUT_MODE>
void launch_trace(uint32_t grid, const rspt_scene_s* s, const TraceCall& c) {
    // XCD-affine dealing (trace_w4.h), RSPT_XCD_DEAL=1: available where the caller hands eight zeroed cursor words (the path integrator's loop, the trace hook).
    // OFF by default: measured neutral to slightly negative (C2 474.0 -> 471.5 Msamples/s, C3 stand-in 2015.6 -> 2014.7; L2 hit rate of the closest-hit
    // launches 0.624 -> 0.620 by TCC_HIT / TCC_MISS — profiles/r05_xcd_affine_ab.txt): the tree's L2 hits are its root side, which every XCD holds anyway
    uint32_t* xcur = (c.xcd_cursors && env_size("RSPT_XCD_DEAL", 0) != 0) ? c.xcd_cursors : nullptr;
    if (s->has_spheres) {   // ABI 23: the sphere instantiations (trace_w4.h SPH)
        launch_trace_sph<ANY, OUT_MODE>(s, c, xcur);
        return;
    }
    static void (*const variants[2][2])(uint32_t, const rspt_scene_s*, const TraceCall&, uint32_t*) = {{launch_trace_v<ANY, OUT_MODE, false, false>, launch_trace_v<ANY, OUT_MODE, false, true>}, {launch_trace_v<ANY, OUT_MODE, true, false>, launch_trace_v<ANY, OUT_MODE, true, true>}};
    variants[s->has_instances][s->has_alpha](grid, s, c, xcur);
}
// ---- the shade-math mode (include/rspt.h rspt_set_shade_math): host-only, process-wide ----
std::atomic<uint32_t> g_shade_math{RSPT_SHADE_MATH_EXACT};
// the mode a render runs under: RSPT_SHADE_MATH = exact | fast when set and non-empty (how an unmodified caller reaches the mode), else what rspt_set_shade_math
// left; -1: the variable holds something else
int shade_math_mode() {
    const char* e = getenv("RSPT_SHADE_MATH");
    if (!e || !*e) return (int)g_shade_math.load();
    if (!strcmp(e, "exact")) return RSPT_SHADE_MATH_EXACT;
    if (!strcmp(e, "fast")) return RSPT_SHADE_MATH_FAST;
    return -1;
}
// ---- the shade stage's instantiations (kernels.h k_shade<F>) ----
// A scene is served by the narrowest compiled feature set that covers what it can put in front of the stage (rspt_scene_s.shade_features
// + the sampler): the code for every other lobe type, light kind, texture slot, instance transform and the Halton sampler folds away,
// and with it registers (generic: 212 VGPRs = 2 waves / SIMD).  The arithmetic that remains is the same, so results do not change.
// (the feature sets SV_DIFFUSE / SV_PLASTIC / SV_TEXTURED / SV_GENERIC: tu_decl.h, next to the instantiations they name)
typedef void (*ShadeKernel)(RSPT_SHADE_ARGS);
// natural = the compiler's own register budget; w3 / w4 = built for 3 / 4 waves per SIMD (amdgpu_waves_per_eu: what does not fit 168 / 128
// VGPRs is spilled); dflt = which of the three runs.  Measured on one box (profiles/r03_ab_shade.md; Msamples/s of C2 / the C3 stand-in,
// k_shade seconds per step): generic 212 VGPRs 423 / 1685 (0.161 / 0.578 s); diffuse 158 VGPRs = 3 waves as compiled 459 (0.111 s), forced to
// 4 waves 455; plastic 173 VGPRs as compiled 1749 (0.531 s), 168 + 24 B of spills = 3 waves 1841 (0.470 s), 128 + 152 B = 4 waves 1791.
struct ShadeVariant { uint32_t features; const char* name; ShadeKernel natural, w3, w4; int dflt; ShadeKernel move; /* the MOVE form (kernels.h PathBuf::move), built as this set's default is; nullptr: none */
                      ShadeKernel f_natural, f_w3, f_w4, f_move; /* the fast-math builds of the same four (kernels.h k_shade_fast*, the SHADE_F* groups of tu_decl.h); nullptr: the set has none */
                      bool sphere_lights; /* the set carries the sphere-light arms (kernels.h k_shade_sl): taken by a sphere scene with an emissive sphere, and by nothing else */
                      bool quadric_lights; /* the set carries the quadric-light arms (kernels.h k_shade_ql): taken by a scene with a disk or a cylinder that serves an area light on a quadric, and by nothing else */ };
// A row names its set once.  _W: a set run at 3 waves by default, its MOVE form built so; W4 = the build behind w4 (the Halton sets have none for 4 waves: 3 again).
// _N: a set run as compiled, its MOVE form too.  Both with their fast-math twins.  _PLAIN: one build, no MOVE form, no fast twins.
#define RSPT_SV_ROW_W(F, NAME, W4) \
    {F, NAME, k_shade<F>, k_shade_w<F, 3>, k_shade_w<F, W4>, 3, k_shade_mw<F, 3>, k_shade_fast<F>, k_shade_fast_w<F, 3>, k_shade_fast_w<F, W4>, k_shade_fast_mw<F, 3>}
#define RSPT_SV_ROW_N(F, NAME) {F, NAME, k_shade<F>, k_shade_w<F, 3>, k_shade_w<F, 4>, 0, k_shade_m<F>, k_shade_fast<F>, k_shade_fast_w<F, 3>, k_shade_fast_w<F, 4>, k_shade_fast_m<F>}
#define RSPT_SV_ROW_PLAIN(F, NAME) {F, NAME, k_shade<F>, k_shade<F>, k_shade<F>, 0, nullptr}
#define RSPT_SV_ROW_SL(F, NAME) {F, NAME, k_shade_sl<F>, k_shade_sl<F>, k_shade_sl<F>, 0, nullptr, nullptr, nullptr, nullptr, nullptr, true}
#define RSPT_SV_ROW_QL(F, NAME) {F, NAME, k_shade_ql<F>, k_shade_ql<F>, k_shade_ql<F>, 0, nullptr, nullptr, nullptr, nullptr, nullptr, false, true}
const ShadeVariant g_shade_variants[] = {
    RSPT_SV_ROW_W(SV_DIFFUSE, "diffuse", 4),   // (round 4: as compiled it now takes 169 VGPRs = 2 waves — the in-kernel voxel claim of light_row_try
                                               //  cost the four registers; the 3-wave build fits 168 without scratch: Cornell 875 -> see profiles/r04_*)
    RSPT_SV_ROW_W(SV_PLASTIC, "plastic", 4),
    RSPT_SV_ROW_N(SV_TEXTURED, "textured"),
    RSPT_SV_ROW_W(SV_DIFFUSE_H, "diffuse-halton", 3),   // (tu_decl.h: the reference's default sampler gets the narrow builds too)
    RSPT_SV_ROW_W(SV_PLASTIC_H, "plastic-halton", 3),
    RSPT_SV_ROW_W(SV_TEXTURED_H, "textured-halton", 3),   // (textured C3 stand-in: 1343 as compiled, 1358 at 3 waves)
    RSPT_SV_ROW_N(SV_GENERIC, "generic"),
    RSPT_SV_ROW_PLAIN(SV_DYNAMIC, "dynamic"),   // (its MOVE form needs 256 VGPRs = one wave per SIMD: dynamic materials keep slots for life)   // + lobe lists built per hit (material_assembly.h)
    RSPT_SV_ROW_PLAIN(SF_ALL, "moving"),        // + moving object instances (dev_scene.h inst_at)
    // scenes with analytic spheres (SF_SPHERE; Sobol' and Halton): the generic / dynamic sets with the sphere arm (dev_bsdf.h shade_sph).  Only
    // sphere scenes take them and sphere scenes take nothing else.  No MOVE form: sphere scenes keep slots for life (the recomputation reads the
    // path's ray by slot).  As compiled: generic-sphere 224 VGPRs, 16 B of scratch, 2 waves / SIMD (generic: 221, 16 B, 2); dynamic-sphere 256 VGPRs
    // + 1 AGPR, 320 B of scratch, ONE wave / SIMD (dynamic: 223, 304 B, 2) — a sphere scene with a dynamic material (a lobe list built per hit: a
    // parameter other than Kd / Ks / roughness varies over the surface) shades at half the occupancy of the triangle set.  Neither rate is measured.
    RSPT_SV_ROW_PLAIN(SV_GENERIC_SPH, "generic-sphere"),
    RSPT_SV_ROW_PLAIN(SV_DYNAMIC_SPH, "dynamic-sphere"),
    // sphere scenes that hold an emissive sphere, while the sphere-light gate is on (rspt_set_sphere_lights): the same two feature sets with the sphere-light
    // arms of shade_path (DiffuseAreaLight over Sphere::sample_with_ref_point / pdf_with_ref_point, dev_sphere_light.h).  Only such renders take them and such
    // renders take nothing else.  No MOVE form, no fast-math form: they run exact under either shade-math mode.  Figures: DESIGN section 5.1a.
    RSPT_SV_ROW_SL(SV_GENERIC_SPH, "generic-spherelight"),
    RSPT_SV_ROW_SL(SV_DYNAMIC_SPH, "dynamic-spherelight"),
    // scenes with a disk or a cylinder (ABI 27, SF_QUADRIC): the two sphere sets with quadric_fill in place of sphere_fill (dev_bsdf.h shade_quad); they serve
    // that scene's spheres and triangles too.  Only such scenes take them and such scenes take nothing else.  Figures: DESIGN section 5.1b.
    RSPT_SV_ROW_PLAIN(SV_GENERIC_QUAD, "generic-quadric"),
    RSPT_SV_ROW_PLAIN(SV_DYNAMIC_QUAD, "dynamic-quadric"),
    // such scenes that hold an emissive disk, cylinder or sphere, while the quadric-light gate is on (rspt_set_quadric_lights; an emissive sphere there needs
    // the sphere-light gate too): the same two feature sets with the quadric-light arms of shade_path (DiffuseAreaLight over the sample_with_ref_point /
    // pdf_with_ref_point of the slot's kind, dev_quadric_light.h).  Only such renders take them and such renders take nothing else.  No MOVE form, no
    // fast-math form: they run exact under either shade-math mode.  Figures: DESIGN section 5.1b.
    RSPT_SV_ROW_QL(SV_GENERIC_QUAD, "generic-quadriclight"),
    RSPT_SV_ROW_QL(SV_DYNAMIC_QUAD, "dynamic-quadriclight"),
    // scenes with a projection or goniometric light (ABI 24, SF_L_MAP; Sobol' and Halton): the generic and the all-features set with the two arms of
    // light_sample_li / light_is_delta (dev_bsdf.h shade_ml).  Only such scenes take them and such scenes take nothing else.  No MOVE form: the
    // schedule was left off for them (unmeasured there), they keep slots for life.
    RSPT_SV_ROW_PLAIN(SV_GENERIC_ML, "generic-maplight"),
    RSPT_SV_ROW_PLAIN(SV_ALL_ML, "all-maplight"),
};
// RSPT_SHADE_VARIANT = name forces an instantiation (it must cover the scene), RSPT_SHADE_WAVES = 0 | 3 | 4 one of its builds (A/B)
// move_out (may be null): the MOVE form of the chosen set when it has one and the build asked for is its default (RSPT_SHADE_WAVES A/B runs stay on the slot-for-life kernels)
// fast (rspt_set_shade_math / RSPT_SHADE_MATH, resolved by the caller): the fast-math builds of the chosen set, picked by the same switches, where the set has them;
// *fast_out then says so.  A set without them (dynamic, moving, sphere, quadric, map-light) is served by its exact kernels: a mode that permits approximation may be exact.
// sphere_lights: the render serves a sphere area light (the caller has checked the gate): only the sets that carry those arms, and they for nothing else
// quadric_lights: the render serves an area light on a quadric in a scene with a disk or a cylinder (the caller has checked the gates): likewise
ShadeKernel shade_kernel_for(uint32_t need, const char** name_out, ShadeKernel* move_out = nullptr, bool fast = false, bool* fast_out = nullptr, bool sphere_lights = false,
                             bool quadric_lights = false) {
    const char* force = getenv("RSPT_SHADE_VARIANT");
    if (move_out) *move_out = nullptr;
    if (fast_out) *fast_out = false;
    const bool sph = (need & SF_SPHERE) != 0, ml = (need & SF_L_MAP) != 0, quad = (need & SF_QUADRIC) != 0;
    for (const ShadeVariant& v : g_shade_variants) {
        if (v.sphere_lights != sphere_lights) continue;
        if (v.quadric_lights != quadric_lights) continue;
        if (shade_sph(v.features) != sph) continue;   // (the triangle sets carry the SF_SPHERE bit too, without the arm: see dev_bsdf.h SF_TRIS_ONLY)
        if (shade_quad(v.features) != quad) continue; // (... and SF_QUADRIC: SF_NO_QUADRIC; a quadric scene's need carries SF_SPHERE too)
        if (shade_ml(v.features) != ml) continue;     // (... and SF_L_MAP: SF_NO_MAPLIGHT)
        if ((need & ~v.features) != 0) continue;
        if (force && *force && strcmp(force, v.name) != 0 && (v.features | SF_DYNAMIC | SF_ANIM) != SF_ALL) continue;
        if (name_out) *name_out = v.name;
        const size_t waves = env_size("RSPT_SHADE_WAVES", (size_t)v.dflt);
        const bool f = fast && v.f_natural != nullptr;
        if (fast_out) *fast_out = f;
        if (move_out && waves == (size_t)v.dflt) *move_out = f ? v.f_move : v.move;
        if (f) return waves == 3 ? v.f_w3 : (waves == 4 ? v.f_w4 : v.f_natural);
        return waves == 3 ? v.w3 : (waves == 4 ? v.w4 : v.natural);
    }
    if (sph || ml) return nullptr;   // (not reached: the dynamic sphere set covers every sphere scene, which never holds moving instances)
    return k_shade<SF_ALL>;
}
