// k_trace_w4pf — the packet walk of trace_packet.h with the per-ray slot tests of the INTERIOR steps replaced by one conservative test of the
// sign group's frustum per record.  k_trace_w4pk runs box_pair_hit_m twice in every masked lane at every record, only to decide whether to
// descend, and the 64 rays through one pixel nearly always answer alike.  Here:
//   * once per sign group, wave reductions give the interval hull of the group's rays: o_lo / o_hi, inv_lo / inv_hi per axis (the signs are
//     fixed inside a group) and tmax_bound = the largest t_max.  Reductions run there and after a leaf phase that recorded a hit, never per step;
//   * at a record, lane k evaluates slot k & 3 alone (six dword loads through one lane-constant offset, 33 VALU instructions per wave and step
//     against ~100): with xn the near and xf the far plane by the group's sign (i > 0: xn = b.min - o_hi, xf = b.max - o_lo; i < 0: xn = b.max - o_lo,
//     xf = b.min - o_hi), L_axis = min(xn * inv_lo, xn * inv_hi), U_axis = max(xf * inv_lo, xf * inv_hi) — evaluated as the min / max of the four
//     products of (b.min - o_hi, b.max - o_lo) with (inv_lo, inv_hi), the same values without a select — L = max3, U = min3 * widen, taken iff
//     L <= U && L < tmax_bound && U > 0; one ballot gives the four slot bits.  Plain float operations, no contraction: rounding
//     is monotone, so L <= every lane's entry distance m and U >= every lane's widened exit distance M of box_pair_hit_m, without an epsilon
//     (tests/test_frustum_bound_host.py restates this in numpy).  A NaN box (an empty slot) gives L = U = NaN and fails L <= U;
//   * the stack holds (ref, L) entries, no lane masks; a popped entry is dropped unread when !(L < tmax_bound);
//   * EVERY leaf, visited directly or popped, is gated: all lanes of the group run box_hit on the leaf's own box (leaf_boxes[first primitive]) with
//     their own t_max, a ballot gives the leaf phase its lanes.
// Exactness.  The reference tests a leaf's triangles iff the leaf's own box passes intersect_p with the ray's t_max of that moment (the ancestors'
// boxes pass whenever it does: monotone in the box, trace_w4.h), and its visiting order depends on the ray only through the group's sign bits.  The
// group walks a superset of its lanes' records in that order (a lane's passing leaf has every ancestor slot taken: L <= m, U >= M, tmax_bound >= t_max),
// and every lane passes the exact gate before a leaf's triangles: each lane sees its reference triangle-test sequence with its own shrinking t_max.
// A group with the literal-chain bit (a zero or non-finite reciprocal) runs the masked walk of trace_packet.h, and so does a group whose hull is wide (origins
// spread over more than 1/16 of the scene's extent, or reciprocals over more than a factor 1.5, on any axis): a hull that wide takes nearly every record, the
// whole tree per group on incoherent rays (tools/trace_bench.py's incoherent set: minutes instead of milliseconds before this rule).
// Everything the kernel writes goes through vector stores (results) and LDS writes (the stack).
#pragma once
#include "trace_packet.h"

namespace rspt {

// wave reductions (64 lanes, butterfly); the result is wave-uniform
RDEV float pf_wave_min(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}
RDEV float pf_wave_max(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

// the interval hull of a sign group's rays: wave-uniform
struct PfHull { float o_lo[3], o_hi[3], inv_lo[3], inv_hi[3]; };
// Only a narrow bundle is walked by its hull: per axis the origins within 1/16 of the scene's extent and the reciprocals within a factor 1.5.  A wide group (incoherent
// rays that merely share their signs) would take nearly every record of the tree; the masked walk serves it.  Either walk is exact, so the choice is one of speed alone.
RDEV bool pf_hull_narrow(const PfHull& h, uint32_t nb, float4 root0, float4 root1) {
    const float ext[3] = {root0.w - root0.x, root1.x - root0.y, root1.y - root0.z};
    bool narrow = true;
    for (int a = 0; a < 3; a++) {
        const bool neg = (nb >> a) & 1u;
        narrow = narrow && (h.o_hi[a] - h.o_lo[a]) * 16.0f <= ext[a] && (neg ? h.inv_lo[a] >= 1.5f * h.inv_hi[a] : h.inv_hi[a] <= 1.5f * h.inv_lo[a]);
    }
    return narrow;
}

// The walk of a group's frustum over the records: `leaf(ref)` gates and serves a leaf and lowers tmax_bound (the largest t_max of the group's rays) after a recorded hit.
// The group's rays are the caller's: 64 of one packet (PfFrustum below) or the 64 R of a bundle (trace_bundle.h).
template <class Leaf>
RDEV void pf_walk_records(const Wide4Node* __restrict__ recs, uint32_t root_ref, uint2* stk, uint32_t lane, uint32_t nb, const PfHull& h, const float& tmax_bound, Leaf& leaf) {
    const float widen = 1.0f + 2.0f * gamma_n(3);
    const float* const o_lo = h.o_lo; const float* const o_hi = h.o_hi; const float* const inv_lo = h.inv_lo; const float* const inv_hi = h.inv_hi;
    uint32_t sp = 0, cur = root_ref;   // (the launch takes this kernel only when the root is an interior record)
    for (;;) {
        if (cur == RSPT_NONE) {
            if (sp == 0) break;
            sp--;
            const uint2 e = stk[sp];
            const uint32_t ref = __builtin_amdgcn_readfirstlane(e.x);
            const float le = __uint_as_float(__builtin_amdgcn_readfirstlane(e.y));
            if (!(le < tmax_bound)) continue;   // no lane of the group can pass a box behind it any more
            if (ref & RSPT_REF_LEAF) {
                leaf(ref);
                continue;
            }
            cur = ref;
        }
        // ---- node step: the record's four slots against the group's frustum, one slot per lane ----
        RSPT_PK_COUNT_ADD(0);
        const char* base = reinterpret_cast<const char*>(recs + cur);
        const float4 rf = pk_load4(reinterpret_cast<const float4*>(base) + 6);
        cur = RSPT_NONE;
        // With a = b.min - o_hi <= b = b.max - o_lo: for i > 0 the near plane is xn = a and the far plane xf = b, for i < 0 xn = b and xf = a, and in both cases
        // min(xn * inv_lo, xn * inv_hi) is the smallest and max(xf * inv_lo, xf * inv_hi) the largest of the four products (x -> x * i is monotone for one i, rounded
        // too): L_axis = min4, U_axis = max4 are the values of the sign-selected form, without a select per lane and axis
        // lane k serves slot k & 3: the byte offset of its min x in a record (Wide4Node: {min s0, min s1, max s0, max s1} per axis, for the pairs (0,1) and (2,3)), worked
        // out here from the lane number (three instructions) and not kept across the leaf phases (two registers)
        uint32_t lk = lane;
        asm volatile("" : "+v"(lk));
        const uint32_t boff = (lk & 2u) * 24u + (lk & 1u) * 4u;
        const float* bp = reinterpret_cast<const float*>(base + boff);
        const float ax = bp[0] - o_hi[0], bx = bp[2] - o_lo[0], ay = bp[4] - o_hi[1], by = bp[6] - o_lo[1], az = bp[8] - o_hi[2], bz = bp[10] - o_lo[2];
        const float pxa = ax * inv_lo[0], pxb = ax * inv_hi[0], pxc = bx * inv_lo[0], pxd = bx * inv_hi[0];
        const float pya = ay * inv_lo[1], pyb = ay * inv_hi[1], pyc = by * inv_lo[1], pyd = by * inv_hi[1];
        const float pza = az * inv_lo[2], pzb = az * inv_hi[2], pzc = bz * inv_lo[2], pzd = bz * inv_hi[2];
        const float lx = fminf(fminf(fminf(pxa, pxb), pxc), pxd), ux = fmaxf(fmaxf(fmaxf(pxa, pxb), pxc), pxd);
        const float ly = fminf(fminf(fminf(pya, pyb), pyc), pyd), uy = fmaxf(fmaxf(fmaxf(pya, pyb), pyc), pyd);
        const float lz = fminf(fminf(fminf(pza, pzb), pzc), pzd), uz = fmaxf(fmaxf(fmaxf(pza, pzb), pzc), pzd);
        const float L = fmaxf(fmaxf(lx, ly), lz);
        const float U = fminf(fminf(ux, uy), uz) * widen;
        const bool taken = (L <= U) && (L < tmax_bound) && (U > 0.0f);
        uint32_t f0 = __builtin_amdgcn_readfirstlane(__float_as_uint(rf.x)), f1 = __builtin_amdgcn_readfirstlane(__float_as_uint(rf.y));
        uint32_t f2 = __builtin_amdgcn_readfirstlane(__float_as_uint(rf.z)), f3w = __builtin_amdgcn_readfirstlane(__float_as_uint(rf.w));
        asm volatile("" : "+s"(f0), "+s"(f1), "+s"(f2), "+s"(f3w));   // (the references are fetched next to the planes, not behind the branch on the ballot: one latency per step, not two)
        const uint32_t bits = (uint32_t)__ballot(taken) & 15u;
        if (bits == 0) continue;
        // the visiting order e0..e3 of the four slots (trace_w4.h: three sign bits), scalar
        const bool sA = ((nb >> ((f0 >> RSPT_W4_AXIS_SHIFT) & 3u)) & 1u) != 0;    // dir_is_neg[A.axis]: second child's subtree first
        const bool sB0 = ((nb >> ((f1 >> RSPT_W4_AXIS_SHIFT) & 3u)) & 1u) != 0;   // order inside the first child
        const bool sB1 = ((nb >> ((f2 >> RSPT_W4_AXIS_SHIFT) & 3u)) & 1u) != 0;   // order inside the second child
        const uint32_t r0 = f0 & ~RSPT_W4_AXIS_MASK, r1 = f1 & ~RSPT_W4_AXIS_MASK, r2 = f2 & ~RSPT_W4_AXIS_MASK, r3 = f3w;
        const uint32_t lb = __float_as_uint(L);
        const uint32_t l0 = (uint32_t)__builtin_amdgcn_readlane((int)lb, 0), l1 = (uint32_t)__builtin_amdgcn_readlane((int)lb, 1);
        const uint32_t l2 = (uint32_t)__builtin_amdgcn_readlane((int)lb, 2), l3 = (uint32_t)__builtin_amdgcn_readlane((int)lb, 3);
        const bool s0 = bits & 1u, s1 = bits & 2u, s2 = bits & 4u, s3 = bits & 8u;
        const uint32_t g0n = sB0 ? r1 : r0, g0f = sB0 ? r0 : r1, g1n = sB1 ? r3 : r2, g1f = sB1 ? r2 : r3;
        const uint32_t d0n = sB0 ? l1 : l0, d0f = sB0 ? l0 : l1, d1n = sB1 ? l3 : l2, d1f = sB1 ? l2 : l3;
        const bool w0n = sB0 ? s1 : s0, w0f = sB0 ? s0 : s1, w1n = sB1 ? s3 : s2, w1f = sB1 ? s2 : s3;
        const uint32_t e0 = sA ? g1n : g0n, e1 = sA ? g1f : g0f, e2 = sA ? g0n : g1n, e3 = sA ? g0f : g1f;
        const uint32_t d1 = sA ? d1f : d0f, d2 = sA ? d0n : d1n, d3 = sA ? d0f : d1f;
        const bool w0 = sA ? w1n : w0n, w1 = sA ? w1f : w0f, w2 = sA ? w0n : w1n, w3 = sA ? w0f : w1f;
        const bool p1 = w0, p2 = p1 || w1, p3 = p2 || w2;   // something earlier in the order is visited first
        const bool push3 = w3 && p3, push2 = w2 && p2, push1 = w1 && p1;
        if (lane == 0) {
            uint32_t q = sp;
            if (push3) stk[q++] = make_uint2(e3, d3);
            if (push2) stk[q++] = make_uint2(e2, d2);
            if (push1) stk[q++] = make_uint2(e1, d1);
        }
        sp += (push3 ? 1u : 0u) + (push2 ? 1u : 0u) + (push1 ? 1u : 0u);
        const uint32_t next = p1 ? e0 : (w1 ? e1 : (w2 ? e2 : e3));
        if (next & RSPT_REF_LEAF) leaf(next);
        else cur = next;
    }
}

// The frustum walk of one sign group without the literal-chain bit (the lanes of gmask, all with negbits == nb), handed to pk_trace_body (trace_packet.h), whose
// per-lane ray state and leaf phase it works on.  Returns false, having walked nothing, for a group that is not a narrow bundle
struct PfFrustum {
    static constexpr bool frustum = true;
    template <class LeafPhase, class LeafRange>
    static RDEV bool walk(const Wide4Node* __restrict__ recs, const float4* __restrict__ leaf_boxes, float4 root0, float4 root1, uint32_t root_ref, uint2* stk, uint32_t lane, uint32_t nb, uint64_t gmask,
                          float ox, float oy, float oz, float ix, float iy, float iz, float& t_max, LeafPhase& leaf_phase, LeafRange& leaf_range) {
        const bool n0 = nb & 1u, n1 = nb & 2u, n2 = nb & 4u;
        const bool ing = ((gmask >> lane) & 1ull) != 0;
        // ---- the group's interval hull (lanes outside the group stay neutral) ----
        const PfHull h = {{pf_wave_min(ing ? ox : RSPT_INF), pf_wave_min(ing ? oy : RSPT_INF), pf_wave_min(ing ? oz : RSPT_INF)},
                          {pf_wave_max(ing ? ox : -RSPT_INF), pf_wave_max(ing ? oy : -RSPT_INF), pf_wave_max(ing ? oz : -RSPT_INF)},
                          {pf_wave_min(ing ? ix : RSPT_INF), pf_wave_min(ing ? iy : RSPT_INF), pf_wave_min(ing ? iz : RSPT_INF)},
                          {pf_wave_max(ing ? ix : -RSPT_INF), pf_wave_max(ing ? iy : -RSPT_INF), pf_wave_max(ing ? iz : -RSPT_INF)}};
        float tmax_bound = pf_wave_max(ing ? t_max : -RSPT_INF);
        if (!pf_hull_narrow(h, nb, root0, root1)) return false;

        // one leaf: the reference's test of the leaf's own box with every lane's t_max of this moment (bvh.rs:424), then its triangles for the lanes that pass
        auto leaf = [&](uint32_t ref) {
            uint32_t offset, n_prims;
            leaf_range(ref, &offset, &n_prims);
            const float4 q0 = pk_load4(leaf_boxes + 2 * (size_t)offset), q1 = pk_load4(leaf_boxes + 2 * (size_t)offset + 1);
            const bool ok = ing && box_hit(q0, q1, f3{ox, oy, oz}, f3{ix, iy, iz}, n0, n1, n2, t_max);
            const uint64_t lmask = __ballot(ok);
            RSPT_PK_COUNT_ADD(1);
            if (lmask == 0) return;
            const float before = t_max;
            leaf_phase(offset, n_prims, lmask);
            if (__ballot(t_max != before)) tmax_bound = pf_wave_max(ing ? t_max : -RSPT_INF);   // (a recorded hit: the group's bound may have dropped)
        };
        pf_walk_records(recs, root_ref, stk, lane, nb, h, tmax_bound, leaf);
        return true;
    }
};

template <int OUT_MODE>
__global__ __launch_bounds__(RSPT_PW_BLOCK) RSPT_PK_ATTR void k_trace_w4pf(RSPT_PK_ARGS) {
    __shared__ uint4 stack_s[RSPT_PK_WAVES * RSPT_W4_MAX_STACK];   // the masked walk: (ref, mask low, mask high, unused); the frustum walk: (ref, L) pairs in the first half of a wave's share
    pk_trace_body<OUT_MODE, PfFrustum>(stack_s + (threadIdx.x >> 6) * RSPT_W4_MAX_STACK, sc, recs, big_leaves, root_ref, queue, count_ptr, count_imm, cursor, rays_a, rays_b, out_a, out_b, out_hits,
                                       chunk, leaf_boxes);
}

}  // namespace rspt
