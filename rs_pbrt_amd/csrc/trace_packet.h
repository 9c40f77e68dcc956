// k_trace_w4pk — closest-hit traversal of plain triangle scenes for launches whose waves hold COHERENT rays: the camera rays of a batch, whose
// pixel-major slot numbering (kernels.h k_raygen) puts 64 samples of one pixel into the 64 lanes of a wave.  k_trace_w4 walks such a wave as 64
// strangers (seven scattered 16-byte loads per lane and step for the same record, a stack and an ordering network per lane, lanes parked at leaves
// on their own).  Here a wave walks ONE stack for its 64 rays:
//   * a packet is 64 consecutive queue entries; lanes are taken in groups of equal negbits (dir_is_neg of the three axes + the "literal compare
//     chain" bit), because the reference's visiting order (bvh.rs:401-461) depends on the ray only through dir_is_neg[axis]: inside a group the
//     order e0..e3 of a record's four slots is the same for every lane and becomes scalar arithmetic;
//   * the current record and a 64-bit lane mask are wave-uniform; the record (and later each triangle) is fetched ONCE per wave through a
//     wave-uniform address (scalar loads); every masked lane runs box_pair_hit_m / box_hit6_m — the functions and operand values of k_trace_w4,
//     hence the same bits — with its own origin, reciprocals and t_max; four ballots give the four slots' lane masks;
//   * the stack holds wave-uniform (ref, mask) entries in LDS (RSPT_W4_MAX_STACK per wave: the walk of a group is one depth-first walk of the tree,
//     so the bound of trace_w4.h holds, and there are no spill rows, no overflow list, no k_trace_fixup).
// Exactness.  Every lane sees a subsequence of the wave's walk — the entries whose mask holds it — in the reference's order, and that subsequence
// is its own reference sequence:
//   * an INTERIOR entry is pushed with the lanes that passed its box at that moment; k_trace_w4 re-checks t_min < t_max on the pop.  Here a lane
//     whose t_max has meanwhile dropped below the entry's t_min is not removed from the mask: it fails all four slot tests of that record (the
//     slots' boxes lie inside the entry's box and Bounds3f::intersect_p is monotone in the box, trace_w4.h), so it tests no triangle the reference
//     does not, and nothing it does is visible;
//   * a LEAF entry popped from the stack needs the reference's test of that moment (a culled lane would otherwise run the leaf's triangles, and a
//     watertight hit outside the shrunken interval is rejected by t_max only up to rounding): every masked lane runs box_hit — the reference's
//     compare chain — on the leaf's own box (leaf_boxes[first primitive], the array k_trace_w4q re-tests leaves with) with its current t_max.  A leaf
//     visited directly as the first slot of the order has just been tested with that t_max;
// Not done (measured, experiments/trace_packet_wave_cull.patch): dropping a popped entry unread when a wave-level lower bound of its entry distances is >=
// the largest t_max of the group — the wave reductions per step cost more than the skipped records saved (C2 camera launch 58.1 against 53.8 ms).
// Everything the kernel writes goes through vector stores (results) and LDS writes (the stack).
#pragma once
#include "trace_w4.h"

namespace rspt {

#define RSPT_PK_WAVES (RSPT_PW_BLOCK / 64)
#ifdef RSPT_PK_OCC   // A/B (tools/ab_build.sh AB_DEFS=-DRSPT_PK_OCC=n): built for n waves per SIMD
#define RSPT_PK_ATTR __attribute__((amdgpu_waves_per_eu(RSPT_PK_OCC, RSPT_PK_OCC)))
#else
#define RSPT_PK_ATTR
#endif

// a wave-uniform fetch: the constant address space + a uniform address selects the scalar data path (one request per wave, not one per lane)
typedef float pk_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t pk_u2 __attribute__((ext_vector_type(2)));
RDEV float4 pk_load4(const float4* p) {
    const pk_f4 v = *reinterpret_cast<const __attribute__((address_space(4))) pk_f4*>(reinterpret_cast<uintptr_t>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
RDEV uint2 pk_load2(const uint2* p) {
    const pk_u2 v = *reinterpret_cast<const __attribute__((address_space(4))) pk_u2*>(reinterpret_cast<uintptr_t>(p));
    return make_uint2(v.x, v.y);
}

#ifdef RSPT_PK_COUNT   // timing-only A/B build (tools/ab_build.sh AB_DEFS=-DRSPT_PK_COUNT): records fetched, leaves tested, packets walked, summed per kernel family
static __device__ unsigned long long g_pk_count[3];   // one copy per translation unit: read where the kernels are instantiated (tu.hip, groups W4PK / W4PF / W4PB)
#define RSPT_PK_COUNT_ADD(i) do { if (__lane_id() == 0) atomicAdd(&g_pk_count[i], 1ull); } while (0)
#else
#define RSPT_PK_COUNT_ADD(i) do { } while (0)
#endif

// k_trace_w4pk walks every sign group with the masked walk below
struct PkMaskedOnly {
    static constexpr bool frustum = false;
    template <class LeafPhase, class LeafRange>
    static RDEV bool walk(const Wide4Node*, const float4*, float4, float4, uint32_t, uint2*, uint32_t, uint32_t, uint64_t, float, float, float, float, float, float, float&, LeafPhase&, LeafRange&) { return false; }
};

// One packet of the packet kernels: lane by lane the queue entry qpos (where `valid`), loaded, walked and stored.  FR::frustum: a sign group without the literal-chain bit is offered to
// FR::walk (trace_frustum.h) first; the masked walk serves the groups it declines.
template <int OUT_MODE, class FR>
RDEV void pk_trace_packet(uint4* stk, const SceneDev& sc, const Wide4Node* __restrict__ recs, const uint2* __restrict__ big_leaves, uint32_t root_ref, const uint32_t* __restrict__ queue,
                          const rspt_ray* __restrict__ rays_a, const rspt_ray* __restrict__ rays_b, float4* __restrict__ out_a, float4* __restrict__ out_b, rspt_hit* __restrict__ out_hits,
                          const float4* __restrict__ leaf_boxes, float4 root0, float4 root1, uint32_t lane, uint32_t qpos, bool valid) {
    {
        // ---- per-lane ray state: the expressions of k_trace_w4's refill block ----
        float ox = 0, oy = 0, oz = 0, ix = 0, iy = 0, iz = 0;
        RayShear rs{0, 0, 0, 0, 0, 0};
        float t_max = 0.0f;
        uint32_t negbits = 0, entry = 0;
        uint32_t best = RSPT_MISS;
        float bt = 0.0f, bb0 = 0.0f, bb1 = 0.0f, bb2 = 0.0f;
        bool alive = false;
        if (valid) {
            entry = queue ? queue[qpos] : qpos;
            const float4* rp = reinterpret_cast<const float4*>(((entry & RSPT_Q_MIS) ? rays_b : rays_a) + (entry & ~RSPT_Q_MIS));
            float4 r0 = rp[0], r1 = rp[1];
            ox = r0.x; oy = r0.y; oz = r0.z;
            f3 d{r0.w, r1.x, r1.y};
            t_max = r1.z;
            ix = 1.0f / d.x; iy = 1.0f / d.y; iz = 1.0f / d.z;
            negbits = (ix < 0.0f ? 1u : 0u) | (iy < 0.0f ? 2u : 0u) | (iz < 0.0f ? 4u : 0u);
            // zero / denormal / NaN direction components: keep the reference's literal compare chain
            if (!(fabsf(ix) < RSPT_INF && fabsf(iy) < RSPT_INF && fabsf(iz) < RSPT_INF)) negbits |= 8u;
            rs = ray_shear(d);
            // the root's own box (bvh.rs:424 on node 0)
            alive = box_hit(root0, root1, f3{ox, oy, oz}, f3{ix, iy, iz}, negbits & 1u, negbits & 2u, negbits & 4u, t_max);
        }

        // ---- the packet's sign groups, one walk each ----
        uint64_t todo = __ballot(alive);
        if (todo) RSPT_PK_COUNT_ADD(2);
        while (todo) {
            const uint32_t nb = (uint32_t)__builtin_amdgcn_readlane((int)negbits, (int)(__ffsll((unsigned long long)todo) - 1));   // wave-uniform
            const uint64_t gmask = __ballot(alive && negbits == nb);
            todo &= ~gmask;
            const bool n0 = nb & 1u, n1 = nb & 2u, n2 = nb & 4u;
            uint32_t sp = 0, cur = root_ref;   // (the launch takes this kernel only when the root is an interior record)
            uint64_t mask = gmask;

            // the triangles of one leaf for the lanes of lmask (trace_w4.h, the leaf phase)
            auto leaf_phase = [&](uint32_t offset, uint32_t n_prims, uint64_t lmask) {
                const bool in = ((lmask >> lane) & 1ull) != 0;
                const f3 o{ox, oy, oz};
                for (uint32_t i = 0; i < n_prims; i++) {
                    const uint32_t pi = offset + i;
                    const float4 a = pk_load4(sc.tris + 3 * (size_t)pi), b = pk_load4(sc.tris + 3 * (size_t)pi + 1), c = pk_load4(sc.tris + 3 * (size_t)pi + 2);
                    float t, b0, b1, b2;
                    if (in && tri_test(f3{a.x, a.y, a.z}, f3{a.w, b.x, b.y}, f3{b.z, b.w, c.x}, o, rs, t_max, &t, &b0, &b1, &b2)) {
                        t_max = t;       // primitive.rs:155: every later box and triangle test sees this
                        best = pi; bt = t; bb0 = b0; bb1 = b1; bb2 = b2;
                    }
                }
            };
            auto leaf_range = [&](uint32_t ref, uint32_t* offset, uint32_t* n_prims) {
                uint32_t off = ref & RSPT_W4_OFFSET_MASK, np = ((ref >> RSPT_W4_COUNT_SHIFT) & 15u) + 1u;
                if (np == 16u) {
                    const uint2 bl = pk_load2(big_leaves + off);
                    off = bl.x; np = bl.y;
                }
                *offset = off; *n_prims = np;
            };

            if (FR::frustum && !(nb & 8u) &&
                FR::walk(recs, leaf_boxes, root0, root1, root_ref, reinterpret_cast<uint2*>(stk), lane, nb, gmask, ox, oy, oz, ix, iy, iz, t_max, leaf_phase, leaf_range))
                continue;   // (false: the group's rays are not a narrow bundle, and nothing was walked)
            for (;;) {
                if (cur == RSPT_NONE) {
                    if (sp == 0) break;
                    sp--;
                    const uint4 e = stk[sp];
                    const uint32_t ref = __builtin_amdgcn_readfirstlane(e.x);
                    mask = (uint64_t)__builtin_amdgcn_readfirstlane(e.y) | ((uint64_t)__builtin_amdgcn_readfirstlane(e.z) << 32);
                    if (ref & RSPT_REF_LEAF) {
                        uint32_t offset, n_prims;
                        leaf_range(ref, &offset, &n_prims);
                        // the reference's test of the leaf's own box at this later moment (bvh.rs:424)
                        const float4 q0 = pk_load4(leaf_boxes + 2 * (size_t)offset), q1 = pk_load4(leaf_boxes + 2 * (size_t)offset + 1);
                        const bool ok = ((mask >> lane) & 1ull) != 0 && box_hit(q0, q1, f3{ox, oy, oz}, f3{ix, iy, iz}, n0, n1, n2, t_max);
                        const uint64_t lmask = __ballot(ok);
                        RSPT_PK_COUNT_ADD(1);
                        if (lmask) leaf_phase(offset, n_prims, lmask);
                        continue;
                    }
                    cur = ref;
                }
                // ---- node step: one record for the lanes of mask ----
                RSPT_PK_COUNT_ADD(0);
                const float4* pp = reinterpret_cast<const float4*>(recs + cur);
                const float4 a0 = pk_load4(pp), a1 = pk_load4(pp + 1), a2 = pk_load4(pp + 2), a3 = pk_load4(pp + 3), a4 = pk_load4(pp + 4), a5 = pk_load4(pp + 5), rf = pk_load4(pp + 6);
                cur = RSPT_NONE;
                const bool in = ((mask >> lane) & 1ull) != 0;
                bool h0, h1, h2, h3;
                float m0, m1, m2, m3;
                if (!FR::frustum && !(nb & 8u)) {   // (under FR::frustum only the literal-chain groups and the wide ones FR::walk declined come here, and take the reference's chain: the pair arm and its registers fold away)
                    box_pair_hit_m(a0, a1, a2, ox, oy, oz, ix, iy, iz, t_max, &h0, &h1, &m0, &m1);
                    __builtin_amdgcn_sched_barrier(0);   // (one pair after the other: interleaved, the two cost ten more registers and a wave of occupancy)
                    box_pair_hit_m(a3, a4, a5, ox, oy, oz, ix, iy, iz, t_max, &h2, &h3, &m2, &m3);
                } else {
                    const f3 o{ox, oy, oz}, inv{ix, iy, iz};
                    h0 = box_hit6_m(a0.x, a1.x, a2.x, a0.z, a1.z, a2.z, o, inv, n0, n1, n2, t_max, &m0);
                    h1 = box_hit6_m(a0.y, a1.y, a2.y, a0.w, a1.w, a2.w, o, inv, n0, n1, n2, t_max, &m1);
                    h2 = box_hit6_m(a3.x, a4.x, a5.x, a3.z, a4.z, a5.z, o, inv, n0, n1, n2, t_max, &m2);
                    h3 = box_hit6_m(a3.y, a4.y, a5.y, a3.w, a4.w, a5.w, o, inv, n0, n1, n2, t_max, &m3);
                }
                h0 = h0 && in; h1 = h1 && in; h2 = h2 && in; h3 = h3 && in;
                const uint64_t s0 = __ballot(h0), s1 = __ballot(h1), s2 = __ballot(h2), s3 = __ballot(h3);
                if ((s0 | s1 | s2 | s3) == 0) continue;
                // the visiting order e0..e3 of the four slots (trace_w4.h: three sign bits), scalar
                const uint32_t f0 = __builtin_amdgcn_readfirstlane(__float_as_uint(rf.x)), f1 = __builtin_amdgcn_readfirstlane(__float_as_uint(rf.y));
                const uint32_t f2 = __builtin_amdgcn_readfirstlane(__float_as_uint(rf.z)), f3w = __builtin_amdgcn_readfirstlane(__float_as_uint(rf.w));
                const bool sA = ((nb >> ((f0 >> RSPT_W4_AXIS_SHIFT) & 3u)) & 1u) != 0;    // dir_is_neg[A.axis]: second child's subtree first
                const bool sB0 = ((nb >> ((f1 >> RSPT_W4_AXIS_SHIFT) & 3u)) & 1u) != 0;   // order inside the first child
                const bool sB1 = ((nb >> ((f2 >> RSPT_W4_AXIS_SHIFT) & 3u)) & 1u) != 0;   // order inside the second child
                const uint32_t r0 = f0 & ~RSPT_W4_AXIS_MASK, r1 = f1 & ~RSPT_W4_AXIS_MASK, r2 = f2 & ~RSPT_W4_AXIS_MASK, r3 = f3w;
                const uint32_t g0n = sB0 ? r1 : r0, g0f = sB0 ? r0 : r1, g1n = sB1 ? r3 : r2, g1f = sB1 ? r2 : r3;
                const uint64_t w0n = sB0 ? s1 : s0, w0f = sB0 ? s0 : s1, w1n = sB1 ? s3 : s2, w1f = sB1 ? s2 : s3;
                const uint32_t e0 = sA ? g1n : g0n, e1 = sA ? g1f : g0f, e2 = sA ? g0n : g1n, e3 = sA ? g0f : g1f;
                const uint64_t w0 = sA ? w1n : w0n, w1 = sA ? w1f : w0f, w2 = sA ? w0n : w1n, w3 = sA ? w0f : w1f;
                const bool p1 = w0 != 0, p2 = p1 || w1 != 0, p3 = p2 || w2 != 0;   // something earlier in the order is visited first
                const bool push3 = w3 != 0 && p3, push2 = w2 != 0 && p2, push1 = w1 != 0 && p1;
                if (lane == 0) {
                    uint32_t q = sp;
                    if (push3) stk[q++] = make_uint4(e3, (uint32_t)w3, (uint32_t)(w3 >> 32), 0u);
                    if (push2) stk[q++] = make_uint4(e2, (uint32_t)w2, (uint32_t)(w2 >> 32), 0u);
                    if (push1) stk[q++] = make_uint4(e1, (uint32_t)w1, (uint32_t)(w1 >> 32), 0u);
                }
                sp += (push3 ? 1u : 0u) + (push2 ? 1u : 0u) + (push1 ? 1u : 0u);
                const uint32_t next = p1 ? e0 : (w1 != 0 ? e1 : (w2 != 0 ? e2 : e3));
                const uint64_t nmask = p1 ? w0 : (w1 != 0 ? w1 : (w2 != 0 ? w2 : w3));
                if (next & RSPT_REF_LEAF) {   // its box has just been tested with the lanes' current t_max
                    uint32_t offset, n_prims;
                    leaf_range(next, &offset, &n_prims);
                    leaf_phase(offset, n_prims, nmask);
                } else {
                    cur = next; mask = nmask;
                }
            }
        }

        // ---- results ----
        if (valid) {
            const uint32_t slot = entry & ~RSPT_Q_MIS;
            if (OUT_MODE == 0) {
                const float4 v = make_float4(__uint_as_float(best), bb0, bb1, bb2);
                if (entry & RSPT_Q_MIS) { out_b[slot] = v; asm volatile(""); }   // (two stores, never one through a selected pointer: that is a flat store)
                else out_a[slot] = v;
            } else {
                rspt_hit h;
                h.prim = best; h.t = bt; h.b0 = bb0; h.b1 = bb1; h.b2 = bb2;
                out_hits[qpos] = h;
            }
        }
    }
}

// The body of the packet kernels: a wave claims runs of the queue and serves them packet by packet.
template <int OUT_MODE, class FR>
RDEV void pk_trace_body(uint4* stk, const SceneDev& sc, const Wide4Node* __restrict__ recs, const uint2* __restrict__ big_leaves, uint32_t root_ref,
                        const uint32_t* __restrict__ queue, const uint32_t* __restrict__ count_ptr, uint32_t count_imm, uint32_t* cursor,
                        const rspt_ray* __restrict__ rays_a, const rspt_ray* __restrict__ rays_b,
                        float4* __restrict__ out_a, float4* __restrict__ out_b, rspt_hit* __restrict__ out_hits,
                        uint32_t chunk /* rays a wave claims per global atomic (a multiple of 64; bit 0 as in trace_w4.h) */,
                        const float4* __restrict__ leaf_boxes) {
    const uint32_t n = count_ptr ? *count_ptr : count_imm;
    {   // a short queue is spread over all waves (trace_w4.h: the claim shrinks to the queue's share per wave)
        const bool adapt = !(chunk & 1u);
        chunk &= ~63u;
        const uint32_t waves = gridDim.x * (uint32_t)RSPT_PK_WAVES;
        uint32_t per = ((n + waves - 1u) / waves + 63u) & ~63u;
        if (per < 64u) per = 64u;
        if (adapt && per < chunk) chunk = per;
    }
    const uint32_t lane = __lane_id();
    const float4 root0 = sc.nodes[0], root1 = sc.nodes[1];
    uint32_t chunk_lo = 0, chunk_hi = 0;   // wave-uniform

    for (;;) {
        // ---- the next packet of the wave's claim ----
        if (chunk_lo == chunk_hi) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(cursor, chunk);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= n) break;
            chunk_lo = base;
            chunk_hi = (n - base) > chunk ? base + chunk : n;
        }
        const uint32_t qpos = chunk_lo + lane;
        const bool valid = qpos < chunk_hi;
        chunk_lo = (chunk_hi - chunk_lo) > 64u ? chunk_lo + 64u : chunk_hi;
        pk_trace_packet<OUT_MODE, FR>(stk, sc, recs, big_leaves, root_ref, queue, rays_a, rays_b, out_a, out_b, out_hits, leaf_boxes, root0, root1, lane, qpos, valid);
    }
}

// The parameters of the three packet kernels (k_trace_w4pk here, k_trace_w4pf in trace_frustum.h, k_trace_w4pb in trace_bundle.h), said once
#define RSPT_PK_ARGS                                                                                                                                            \
    SceneDev sc, const Wide4Node* __restrict__ recs, const uint2* __restrict__ big_leaves, uint32_t root_ref, const uint32_t* __restrict__ queue,                \
        const uint32_t* __restrict__ count_ptr, uint32_t count_imm, uint32_t* cursor, const rspt_ray* __restrict__ rays_a, const rspt_ray* __restrict__ rays_b,  \
        float4* __restrict__ out_a, float4* __restrict__ out_b, rspt_hit* __restrict__ out_hits, uint32_t chunk, const float4* __restrict__ leaf_boxes
template <int OUT_MODE>
__global__ __launch_bounds__(RSPT_PW_BLOCK) RSPT_PK_ATTR void k_trace_w4pk(RSPT_PK_ARGS) {
    __shared__ uint4 stack_s[RSPT_PK_WAVES * RSPT_W4_MAX_STACK];   // (ref, mask low, mask high, unused)
    pk_trace_body<OUT_MODE, PkMaskedOnly>(stack_s + (threadIdx.x >> 6) * RSPT_W4_MAX_STACK, sc, recs, big_leaves, root_ref, queue, count_ptr, count_imm, cursor, rays_a, rays_b, out_a, out_b, out_hits,
                                          chunk, leaf_boxes);
}

}  // namespace rspt
