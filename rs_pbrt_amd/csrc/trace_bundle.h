// k_trace_w4pb<OUT_MODE, R> — the frustum walk of trace_frustum.h for a BUNDLE of R packets per wave.  k_raygen numbers slots pixel-major, so with 64 R or more samples per
// pixel the R consecutive packets of a wave's claim look through one pixel: they walk the same records, pass the same leaf gates and fetch the same triangles, R times
// over.  Here a wave takes 64 R consecutive queue entries, lane l holding the R rays base + 64 r + l ("set" r), and walks the tree once for all of them:
//   * sign groups are formed over all 64 R rays (one lane mask per set); the group's hull (PfHull) and tmax_bound are reduced over the R sets per lane first, then over the wave;
//   * the node walk is pf_walk_records, the walk k_trace_w4pf runs: one slot per lane, (ref, L) stack entries, one dependent fetch per step — for 64 R rays;
//   * at a leaf its box and its triangles are fetched once; set after set, the lanes of the group run the reference's box_hit on the leaf's own box with their own t_max of that
//     moment, and those that pass run tri_test.  tmax_bound is recomputed only after a recorded hit.
// Exactness is trace_frustum.h's argument over more rays: the visiting order depends on a ray only through the group's sign bits; the group walks a superset of every ray's
// records (L <= m, U >= M, tmax_bound >= t_max); every ray passes the exact gate with its own t_max before a leaf's triangles.  A ray's triangle tests inside a leaf run in the
// leaf's order whatever the other sets do, so each of the 64 R rays sees its reference triangle-test sequence.
// A bundle that holds a literal-chain ray (negbits & 8) or a sign group that is not narrow (pf_hull_narrow over the whole bundle: packets of distant pixels, incoherent rays)
// is handed packet by packet to pk_trace_packet<PfFrustum>, the code of k_trace_w4pf, before anything of it is walked: results and cost of those packets are that kernel's.
// The R ray sets are indexed by compile-time constants only (unrolled loops): a run-time index would send them to scratch.
// Everything the kernel writes goes through vector stores (results) and LDS writes (the stack).
#pragma once
#include "trace_frustum.h"

namespace rspt {

#ifdef RSPT_PK_COUNT
#define RSPT_PB_COUNT_BUNDLE() RSPT_PK_COUNT_ADD(2)
#else
#define RSPT_PB_COUNT_BUNDLE() do { } while (0)
#endif

// the R rays of a lane
template <int R>
struct PbRays {
    float ox[R], oy[R], oz[R], ix[R], iy[R], iz[R], t_max[R];
    int kz[R];   // RayShear; kx and ky follow from kz and are worked out where a triangle is tested
    float sx[R], sy[R], sz[R];
    uint32_t best[R];
    float bt[R], bb0[R], bb1[R], bb2[R];
};

// dir_is_neg of the three axes (a bundle with a literal-chain ray never gets here: no fourth bit)
RDEV uint32_t pb_negbits(float ix, float iy, float iz) { return (ix < 0.0f ? 1u : 0u) | (iy < 0.0f ? 2u : 0u) | (iz < 0.0f ? 4u : 0u); }

// the hull of the rays of gm[] (one lane mask per set) and the largest of their t_max
template <int R>
RDEV PfHull pb_hull(const PbRays<R>& q, const uint64_t (&gm)[R], uint32_t lane) {
    float lo[6], hi[6];
    for (int k = 0; k < 6; k++) { lo[k] = RSPT_INF; hi[k] = -RSPT_INF; }
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (!((gm[r] >> lane) & 1ull)) continue;
        const float v[6] = {q.ox[r], q.oy[r], q.oz[r], q.ix[r], q.iy[r], q.iz[r]};
        for (int k = 0; k < 6; k++) { lo[k] = fminf(lo[k], v[k]); hi[k] = fmaxf(hi[k], v[k]); }
    }
    return PfHull{{pf_wave_min(lo[0]), pf_wave_min(lo[1]), pf_wave_min(lo[2])}, {pf_wave_max(hi[0]), pf_wave_max(hi[1]), pf_wave_max(hi[2])},
                  {pf_wave_min(lo[3]), pf_wave_min(lo[4]), pf_wave_min(lo[5])}, {pf_wave_max(hi[3]), pf_wave_max(hi[4]), pf_wave_max(hi[5])}};
}
template <int R>
RDEV float pb_tmax_bound(const PbRays<R>& q, const uint64_t (&gm)[R], uint32_t lane) {
    float m = -RSPT_INF;
#pragma unroll
    for (int r = 0; r < R; r++) m = ((gm[r] >> lane) & 1ull) ? fmaxf(m, q.t_max[r]) : m;
    return pf_wave_max(m);
}
// the next sign group of todo[] (the rays not yet served): its sign bits and its lane masks, taken out of todo[]
template <int R>
RDEV uint32_t pb_next_group(const PbRays<R>& q, uint64_t (&todo)[R], uint64_t (&gm)[R]) {
    uint32_t nb = 0;
    bool found = false;
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (!found && todo[r]) {
            nb = (uint32_t)__builtin_amdgcn_readlane((int)pb_negbits(q.ix[r], q.iy[r], q.iz[r]), (int)(__ffsll((unsigned long long)todo[r]) - 1));   // wave-uniform
            found = true;
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        gm[r] = todo[r] & __ballot(pb_negbits(q.ix[r], q.iy[r], q.iz[r]) == nb);
        todo[r] &= ~gm[r];
    }
    return nb;
}

template <int OUT_MODE, int R>
__global__ __launch_bounds__(RSPT_PW_BLOCK) RSPT_PK_ATTR void k_trace_w4pb(RSPT_PK_ARGS) {
    __shared__ uint4 stack_s[RSPT_PK_WAVES * RSPT_W4_MAX_STACK];   // a packet handed to pk_trace_packet: as in k_trace_w4pf; the bundle walk: (ref, L) pairs in the first half of a wave's share
    uint4* const stk = stack_s + (threadIdx.x >> 6) * RSPT_W4_MAX_STACK;
    constexpr uint32_t BUNDLE = 64u * R;
    const uint32_t n = count_ptr ? *count_ptr : count_imm;
    {   // a short queue is spread over all waves (trace_w4.h), in whole bundles: a claim starts at a multiple of 64 R, so that bundles are whole pixels where a pixel has 64 R samples
        const bool adapt = !(chunk & 1u);
        chunk &= ~(BUNDLE - 1u);
        if (chunk < BUNDLE) chunk = BUNDLE;
        const uint32_t waves = gridDim.x * (uint32_t)RSPT_PK_WAVES;
        uint32_t per = ((n + waves - 1u) / waves + (BUNDLE - 1u)) & ~(BUNDLE - 1u);
        if (per < BUNDLE) per = BUNDLE;
        if (adapt && per < chunk) chunk = per;
    }
    const uint32_t lane = __lane_id();
    const float4 root0 = sc.nodes[0], root1 = sc.nodes[1];
    uint32_t chunk_lo = 0, chunk_hi = 0;   // wave-uniform

    for (;;) {
        // ---- the next bundle of the wave's claim ----
        if (chunk_lo == chunk_hi) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(cursor, chunk);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= n) break;
            chunk_lo = base;
            chunk_hi = (n - base) > chunk ? base + chunk : n;
        }
        const uint32_t first = chunk_lo;
        chunk_lo = (chunk_hi - chunk_lo) > BUNDLE ? chunk_lo + BUNDLE : chunk_hi;

        // ---- per-ray state: the expressions of pk_trace_packet's refill block, once per set ----
        PbRays<R> q;
        uint64_t todo[R];   // the set's lanes whose ray passed the root's box
        bool chain = false;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t qpos = first + 64u * r + lane;
            q.ox[r] = q.oy[r] = q.oz[r] = q.ix[r] = q.iy[r] = q.iz[r] = q.t_max[r] = 0.0f;
            q.kz[r] = 0; q.sx[r] = q.sy[r] = q.sz[r] = 0.0f;
            q.best[r] = RSPT_MISS;
            q.bt[r] = q.bb0[r] = q.bb1[r] = q.bb2[r] = 0.0f;
            bool alive = false;
            if (qpos < chunk_hi) {
                const uint32_t entry = queue ? queue[qpos] : qpos;
                const float4* rp = reinterpret_cast<const float4*>(((entry & RSPT_Q_MIS) ? rays_b : rays_a) + (entry & ~RSPT_Q_MIS));
                float4 r0 = rp[0], r1 = rp[1];
                q.ox[r] = r0.x; q.oy[r] = r0.y; q.oz[r] = r0.z;
                f3 d{r0.w, r1.x, r1.y};
                q.t_max[r] = r1.z;
                q.ix[r] = 1.0f / d.x; q.iy[r] = 1.0f / d.y; q.iz[r] = 1.0f / d.z;
                const uint32_t negbits = pb_negbits(q.ix[r], q.iy[r], q.iz[r]);
                // zero / denormal / NaN direction components: the reference's literal compare chain, which the packet code keeps
                if (!(fabsf(q.ix[r]) < RSPT_INF && fabsf(q.iy[r]) < RSPT_INF && fabsf(q.iz[r]) < RSPT_INF)) chain = true;
                const RayShear rs = ray_shear(d);
                q.kz[r] = rs.kz; q.sx[r] = rs.sx; q.sy[r] = rs.sy; q.sz[r] = rs.sz;
                // the root's own box (bvh.rs:424 on node 0)
                alive = box_hit(root0, root1, f3{q.ox[r], q.oy[r], q.oz[r]}, f3{q.ix[r], q.iy[r], q.iz[r]}, negbits & 1u, negbits & 2u, negbits & 4u, q.t_max[r]);
            }
            todo[r] = __ballot(alive);
            __builtin_amdgcn_sched_barrier(0);   // (one set after the other, here and at the leaves: interleaved, the sets cost twelve registers more)
        }

        // ---- does the bundle qualify?  No literal-chain ray (alive or not: its set's signs would not be its negbits), every sign group a narrow bundle ----
        bool whole = __ballot(chain) == 0;
        uint64_t gm[R];
        uint32_t nb = 0;
        PfHull h{};
        bool any = false;
        if (whole) {
            uint64_t rest[R];
#pragma unroll
            for (int r = 0; r < R; r++) { rest[r] = todo[r]; any = any || todo[r] != 0; }
            if (any) {   // the first group's hull is kept for its walk: nearly every bundle of a camera launch is one group
                nb = pb_next_group<R>(q, rest, gm);
                h = pb_hull<R>(q, gm, lane);
                whole = pf_hull_narrow(h, nb, root0, root1);
#pragma unroll
                for (int r = 0; r < R; r++) todo[r] = rest[r];
                for (;;) {   // the other groups
                    bool more = false;
#pragma unroll
                    for (int r = 0; r < R; r++) more = more || rest[r] != 0;
                    if (!whole || !more) break;
                    uint64_t gx[R];
                    const uint32_t nx = pb_next_group<R>(q, rest, gx);
                    whole = pf_hull_narrow(pb_hull<R>(q, gx, lane), nx, root0, root1);
                }
            }
        }
        if (!whole) {   // packet by packet through the code of k_trace_w4pf (a run-time loop: one copy of that code)
#pragma unroll 1
            for (uint32_t p = first; p < chunk_lo; p += 64u)
                pk_trace_packet<OUT_MODE, PfFrustum>(stk, sc, recs, big_leaves, root_ref, queue, rays_a, rays_b, out_a, out_b, out_hits, leaf_boxes, root0, root1, lane, p + lane, p + lane < chunk_hi);
            continue;
        }

        // ---- the bundle's sign groups, one walk each ----
        if (any) RSPT_PB_COUNT_BUNDLE();
        while (any) {
            const bool n0 = nb & 1u, n1 = nb & 2u, n2 = nb & 4u;
            float tmax_bound = pb_tmax_bound<R>(q, gm, lane);
            // one leaf: its box and its triangles fetched once; set after set the reference's test of the leaf's own box with every ray's t_max of this moment (bvh.rs:424), then
            // the triangles for the rays that pass (trace_w4.h, the leaf phase)
            auto leaf = [&](uint32_t ref) {
                uint32_t offset = ref & RSPT_W4_OFFSET_MASK, n_prims = ((ref >> RSPT_W4_COUNT_SHIFT) & 15u) + 1u;
                if (n_prims == 16u) {
                    const uint2 bl = pk_load2(big_leaves + offset);
                    offset = bl.x; n_prims = bl.y;
                }
                const float4 q0 = pk_load4(leaf_boxes + 2 * (size_t)offset), q1 = pk_load4(leaf_boxes + 2 * (size_t)offset + 1);
                uint64_t lm[R], lany = 0;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const bool ok = ((gm[r] >> lane) & 1ull) != 0 && box_hit(q0, q1, f3{q.ox[r], q.oy[r], q.oz[r]}, f3{q.ix[r], q.iy[r], q.iz[r]}, n0, n1, n2, q.t_max[r]);
                    lm[r] = __ballot(ok);
                    __builtin_amdgcn_sched_barrier(0);
                    lany |= lm[r];
                }
                RSPT_PK_COUNT_ADD(1);
                if (lany == 0) return;
                bool hit = false;
                for (uint32_t i = 0; i < n_prims; i++) {
                    const uint32_t pi = offset + i;
                    const float4 a = pk_load4(sc.tris + 3 * (size_t)pi), b = pk_load4(sc.tris + 3 * (size_t)pi + 1), c = pk_load4(sc.tris + 3 * (size_t)pi + 2);
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        if (lm[r] == 0) continue;   // wave-uniform
                        float t, b0, b1, b2;
                        RayShear rs{0, 0, q.kz[r], q.sx[r], q.sy[r], q.sz[r]};
                        rs.kx = rs.kz + 1; if (rs.kx == 3) rs.kx = 0;   // (ray_shear's own expressions)
                        rs.ky = rs.kx + 1; if (rs.ky == 3) rs.ky = 0;
                        if (((lm[r] >> lane) & 1ull) != 0 &&
                            tri_test(f3{a.x, a.y, a.z}, f3{a.w, b.x, b.y}, f3{b.z, b.w, c.x}, f3{q.ox[r], q.oy[r], q.oz[r]}, rs, q.t_max[r], &t, &b0, &b1, &b2)) {
                            q.t_max[r] = t;       // primitive.rs:155: every later box and triangle test of this ray sees this
                            q.best[r] = pi; q.bb0[r] = b0; q.bb1[r] = b1; q.bb2[r] = b2;
                            if (OUT_MODE == 1) q.bt[r] = t;
                            hit = true;
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if (__ballot(hit)) tmax_bound = pb_tmax_bound<R>(q, gm, lane);   // (a recorded hit: the group's bound may have dropped)
            };
            pf_walk_records(recs, root_ref, reinterpret_cast<uint2*>(stk), lane, nb, h, tmax_bound, leaf);

            any = false;
#pragma unroll
            for (int r = 0; r < R; r++) any = any || todo[r] != 0;
            if (any) {
                nb = pb_next_group<R>(q, todo, gm);
                h = pb_hull<R>(q, gm, lane);
            }
        }

        // ---- results (the entry is read again here, not kept across the walk: a register per set) ----
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t qpos = first + 64u * r + lane;
            if (qpos < chunk_hi) {
                if (OUT_MODE == 0) {
                    const uint32_t entry = queue ? queue[qpos] : qpos;
                    const uint32_t slot = entry & ~RSPT_Q_MIS;
                    const float4 v = make_float4(__uint_as_float(q.best[r]), q.bb0[r], q.bb1[r], q.bb2[r]);
                    if (entry & RSPT_Q_MIS) { out_b[slot] = v; asm volatile(""); }   // (two stores, never one through a selected pointer: that is a flat store)
                    else out_a[slot] = v;
                } else {
                    rspt_hit hr;
                    hr.prim = q.best[r]; hr.t = q.bt[r]; hr.b0 = q.bb0[r]; hr.b1 = q.bb1[r]; hr.b2 = q.bb2[r];
                    out_hits[qpos] = hr;
                }
            }
        }
    }
}

}  // namespace rspt
