// k_trace_w4 — the production traversal kernel (K2/K3): persistent waves, dynamic ray fetch,
// four-boxes-per-record BVH nodes, entry distances on the stack, deferred leaf phase.
//
// Like k_trace_pw (trace_wide.h) it produces, for every ray, exactly the triangle-test sequence
// of BVHAccel::intersect / intersect_p (bvh.rs:401-514) — near child first by dir_is_neg[axis],
// the shrinking t_max applied to every later box and triangle test — so (prim, t, b0, b1, b2) are
// bit-identical to the reference, ties included.  Two things are done differently from k_trace_pw:
//
//   * One 128-byte record per interior node A at even depth holds the boxes of A's grandchildren
//     (or of a child that is a leaf): slots 0,1 = children of A's first child, slots 2,3 = children
//     of A's second child.  The reference visits them in the order fixed by three sign bits
//     (dir_is_neg[A.axis] picks the group, dir_is_neg[child.axis] the order inside a group).  The
//     skipped intermediate box test is redundant: a grandchild's box lies inside its parent's box
//     and Bounds3f::intersect_p (geometry.rs:2211-2269) is monotone in the box (same products,
//     monotone rounding), so a ray that reaches a grandchild's box also passes the parent's.
//     Halving the number of dependent fetch + pop/push rounds is what pays: the kernel is bound by
//     the L1 request rate of its per-lane record loads (seven per step) and VALU issue, not by
//     bytes.
//   * intersect_p depends on ray.t_max only through its last comparison `t_min < ray.t_max`.  The
//     stack therefore keeps (ref, t_min) and a pop re-checks `t_min < t_max` — exactly the outcome
//     of the reference's box test at the later moment (with the smaller t_max) — without fetching
//     the node again.  Entries whose box failed the t_max-independent part are never pushed.
//
// Leaf refs carry (first primitive, count) so the leaf phase needs no LinearBVHNode fetch.
#pragma once
#include "trace_wide.h"
#include "dev_quadric.h"

namespace rspt {

struct Wide4Node {      // 128 B, 128-byte aligned
    float4 b[6];        // b[0..2]: x, y, z slabs of slots 0,1 as (s0.min, s1.min, s0.max, s1.max); b[3..5]: slots 2,3
    uint32_t ref[4];    // bit 31 = leaf (RSPT_W4_* fields), else Wide4Node index; empty slots have a NaN box (ref never read).
                        // Bits 25..26 of ref[0], ref[1], ref[2] carry A.axis, the first child's axis and the second child's
                        // axis: the kernel is bound by the number of scattered load instructions per step (one more dword
                        // load per step cost 10 % of the kernel's time), so the axes ride in the load that fetches the refs.
    uint32_t pad[4];
};
// leaf ref: bit 31 | (count - 1) << 27 | first primitive; count field 15 = look the pair up in big_leaves[low bits]
#define RSPT_W4_COUNT_SHIFT 27
#define RSPT_W4_AXIS_SHIFT 25
#define RSPT_W4_AXIS_MASK 0x06000000u
#define RSPT_W4_OFFSET_MASK 0x01ffffffu
#define RSPT_W4_ENTER 0xfffffffeu   // k_trace_w4<.., ANIM>: "parked in front of an instance" in the lane's leaf word (no leaf reference carries the axis bits)
#ifndef RSPT_W4_LDS
#define RSPT_W4_LDS 12       // stack entries per lane (8 B each) kept in LDS: 24 KB per workgroup
#endif
#ifndef RSPT_W4_TOP
#define RSPT_W4_TOP 56       // records nearest the root (a breadth-first prefix, numbered first by scene_records.h build_w4) that every
                             // workgroup keeps in LDS: their fetches leave the L1 request path that bounds the kernel.
                             // 2048 * RSPT_W4_LDS + 112 * RSPT_W4_TOP must stay under ~31 KB or only four workgroups fit a CU
                             // (measured C2 / C3 Msamples/s: (16, 0) 366 / 1139; (12, 56) 379 / 1172; (11, 72) 382 / 1161;
                             //  (10, 85) 381 / 1153; (13, 36) 378 / 1170; four workgroups (12, 72) 375 / 1137; three (16, 85) 340 / 1065;
                             //  six waves per SIMD forced with amdgpu_waves_per_eu (80 VGPRs, 13 spilled) and (10, 56): 366 / 1141)
#endif
static_assert(2048 * RSPT_W4_LDS + 112 * RSPT_W4_TOP <= 64 * 1024, "k_trace_w4 LDS budget (64 KB per workgroup)");
#define RSPT_W4_TOP_MAX 512  // the breadth-first prefix scene_records.h build_w4 numbers first: the largest TOPCAP any instantiation keeps in LDS
#ifndef RSPT_W4_SHAPE_DEFAULT
#define RSPT_W4_SHAPE_DEFAULT 0
#endif
#ifndef RSPT_W4_POP_TRIES
#define RSPT_W4_POP_TRIES 1  // stack entries a lane may discard (t_min >= t_max) in one iteration before it gives up the slot
#endif
#ifndef RSPT_W4_STEPS
#define RSPT_W4_STEPS 2      // node steps per outer iteration (refill / leaf-phase checks in between); measured on C2 / C3:
                             // (tries, steps) = (1,1) 334.5 / 1059, (3,1) 326.9 / 1041, (1,2) 338.5 / 1073, (3,2) 333.7 / 1049 Msamples/s
#endif
#define RSPT_W4_MAX_STACK 96 // deepest stack a ray can need: rspt_scene_create admits at most 64 LinearBVHNode levels (the reference's own
                             // fixed stack, bvh.rs:420) = 32 record levels, and a step leaves at most three entries behind per level
#define RSPT_W4_SPILL (RSPT_W4_MAX_STACK - RSPT_W4_LDS)  // further entries per lane in a global spill buffer (spill_rows <= this): with all of
                             // them no ray can overflow, so no ray is re-traced from scratch (round 1 stopped at 48 rows and paid 132 ms
                             // per C2 frame for a handful of deep rays redone one per lane by k_trace_fixup); fewer rows
                             // (RSPT_W4_SPILL_ROWS) bring k_trace_fixup back

// box_pair_hit (trace_wide.h) that also returns the entry distances
RDEV void box_pair_hit_m(float4 q0, float4 q1, float4 q2, float ox, float oy, float oz, float ix, float iy, float iz, float ray_tmax,
                         bool* h0, bool* h1, float* m0o, float* m1o) {
    const float widen = 1.0f + 2.0f * gamma_n(3);
    v2f lx = (v2f{q0.x, q0.y} - ox) * ix, hx = (v2f{q0.z, q0.w} - ox) * ix;
    v2f ly = (v2f{q1.x, q1.y} - oy) * iy, hy = (v2f{q1.z, q1.w} - oy) * iy;
    v2f lz = (v2f{q2.x, q2.y} - oz) * iz, hz = (v2f{q2.z, q2.w} - oz) * iz;
    // x -> x * widen is monotone, so min3 of the widened fars == widened min3 of the fars (one multiply instead of three)
    float m0 = fmaxf(fmaxf(fminf(lx.x, hx.x), fminf(ly.x, hy.x)), fminf(lz.x, hz.x));
    float m1 = fmaxf(fmaxf(fminf(lx.y, hx.y), fminf(ly.y, hy.y)), fminf(lz.y, hz.y));
    v2f M = v2f{fminf(fminf(fmaxf(lx.x, hx.x), fmaxf(ly.x, hy.x)), fmaxf(lz.x, hz.x)),
                fminf(fminf(fmaxf(lx.y, hx.y), fmaxf(ly.y, hy.y)), fmaxf(lz.y, hz.y))} * widen;
    *h0 = (m0 <= M.x) && (m0 < ray_tmax) && (M.x > 0.0f);
    *h1 = (m1 <= M.y) && (m1 < ray_tmax) && (M.y > 0.0f);
    *m0o = m0; *m1o = m1;
}
// literal reference chain (zero / non-finite direction components), returning the final t_min
RDEVN bool box_hit6_m(float lx, float ly, float lz, float hx, float hy, float hz, f3 o, f3 inv, bool ng0, bool ng1, bool ng2, float ray_tmax, float* mo) {
    const float widen = 1.0f + 2.0f * gamma_n(3);
    float t_min = ((ng0 ? hx : lx) - o.x) * inv.x;
    float t_max = ((ng0 ? lx : hx) - o.x) * inv.x;
    float ty_min = ((ng1 ? hy : ly) - o.y) * inv.y;
    float ty_max = ((ng1 ? ly : hy) - o.y) * inv.y;
    t_max *= widen;
    ty_max *= widen;
    *mo = 0.0f;
    if (t_min > ty_max || ty_min > t_max) return false;
    if (ty_min > t_min) t_min = ty_min;
    if (ty_max < t_max) t_max = ty_max;
    float tz_min = ((ng2 ? hz : lz) - o.z) * inv.z;
    float tz_max = ((ng2 ? lz : hz) - o.z) * inv.z;
    tz_max *= widen;
    if (t_min > tz_max || tz_min > t_max) return false;
    if (tz_min > t_min) t_min = tz_min;
    if (tz_max < t_max) t_max = tz_max;
    *mo = t_min;
    return (t_min < ray_tmax) && (t_max > 0.0f);
}

// INST (scenes with object instances): a leaf primitive may be a TransformedPrimitive (primitive.rs:216-265).  The lane
// then pushes the reference to the rest of that leaf, switches to the instance's object-space ray (Transform::transform_ray with
// m_inv), runs the object's own records on top of the same stack, and on coming back down to that stack level reloads the world
// ray from its queue record.  t_max is carried over as the reference does (r.t_max.set(ray.t_max), quirks Q10 / Q11 in kernels.h
// traverse<>).  Without INST the code is the one measured in DESIGN.md (the flag is a template parameter, not a branch).
// ALPHA (scenes with alpha-masked meshes): a candidate that passed the watertight test on such a mesh is checked by alpha_pass
// (kernels.h) before it counts — a call into the texture code, which is why this too is a template flag.
// ANIM (with INST): some instances move (AnimatedTransform primitive_to_world, primitive.rs:198-222): entering such an instance interpolates its Transform at the
// ray's time (dev_scene.h inst_at — two key decompositions blended, a 4x4 inverse: ~100 live values for a moment), so it is its own instantiation and every
// other instanced scene keeps the register budget it was measured with.
// BLOCK / TOPCAP (round 5): threads per workgroup and the number of root-side records a workgroup keeps in LDS.  The measured default is five 256-thread
// workgroups per CU with 56 records each (30 KB); ONE 1024-thread workgroup per CU has room for 512 (96 KB of stack columns + 56 KB of records = the CU's
// 160 KB, declared as dynamic LDS): a ninth of the record fetches of an incoherent ray come from the first 56 records, about a quarter from the first 512 —
// fetches that leave the L1 request path the kernel is bound by.
#ifdef RSPT_W4_WAVES   // A/B (tools/ab_build.sh AB_DEFS=-DRSPT_W4_WAVES=n): every instantiation built for n waves per SIMD (what does not fit the budget is spilled)
#define RSPT_W4_ATTR __attribute__((amdgpu_waves_per_eu(RSPT_W4_WAVES, RSPT_W4_WAVES)))
#else
// the closest-hit kernel over moving instances is built for FOUR waves per SIMD: 147 -> 128 VGPRs + 64 B of scratch around the entry phase; all-moving C5 stand-in 183.2 -> 199.4
// Msamples/s (two alternating rounds, profiles/r06_c5_anim_waves_ab.txt).  (1, 8) is the backend's own default: every other instantiation keeps the budget it was measured with.
#define RSPT_W4_ATTR __attribute__((amdgpu_waves_per_eu((ANIM && !ANY) ? 4 : 1, (ANIM && !ANY) ? 4 : 8)))
#endif
// SPH (ABI 23, scenes with spheres; never with INST): a leaf record carrying MF_SPHERE is a GeometricPrimitive over a Sphere — dev_sphere.h sphere_test
// (Sphere::intersect / intersect_p up to t_shape_hit) on the world ray, reloaded from its queue record for the direction; its t becomes the ray's t_max
// (primitive.rs:150-156).  A sphere hit writes its primitive and its t: the hook's rspt_hit has t and b0..b2 = 0; the render's queue record
// (OUT_MODE 0) is (prim, t, 0, 0), the shade stage recomputing the interaction (kernels.h sphere_fill).  The triangle instantiations (SPH = false) compile none of it.
// QUAD (ABI 27, scenes with a disk or a cylinder; always with SPH): the record behind an MF_SPHERE leaf entry is a QuadricDev (dev_quadric.h) whose kind picks the test.
// Those scenes take k_trace_w4quad below, which serves their spheres and triangles too; k_trace_w4<.., SPH> keeps calling sphere_test and so keeps its code.
template <bool QUAD>
RDEV bool w4_quadric_leaf(const SphereDev* rec, f3 o, f3 d, float t_max, float* t_out) {
    if constexpr (QUAD) return quadric_test(*reinterpret_cast<const QuadricDev*>(rec), o, d, t_max, t_out);
    else return sphere_test(rec->s, o, d, t_max, t_out);
}
// The parameters of k_trace_w4 and k_trace_w4quad, said once: the definitions here, the instantiations of tu_decl.h.  chunk: rays a wave claims per global atomic (a multiple of 64)
#define RSPT_W4_ARGS                                                                                                                                                  \
    SceneDev sc, TexTables tt, const Wide4Node* __restrict__ recs, const uint2* __restrict__ big_leaves, uint32_t root_ref, const uint32_t* __restrict__ queue,        \
        const uint32_t* __restrict__ count_ptr, uint32_t count_imm, uint32_t* cursor, const rspt_ray* __restrict__ rays_a, const rspt_ray* __restrict__ rays_b,        \
        float4* __restrict__ out_a, float4* __restrict__ out_b, uint32_t* __restrict__ out_occ, rspt_hit* __restrict__ out_hits, uint32_t* n_overflow,                 \
        uint32_t* __restrict__ overflow_list, uint2* __restrict__ spill, uint32_t spill_rows, int refill_thresh, int leaf_thresh, uint32_t n_top,                      \
        uint32_t* __restrict__ out_inst, uint32_t* xcd_cursors, uint32_t chunk
template <bool ANY, int OUT_MODE, bool INST, int ALPHA /* 0: no masks, 1: alpha_pass (any texture graph, a call), 2: alpha_simple (in line) */, bool ANIM = false,
          int BLOCK = RSPT_PW_BLOCK, int TOPCAP = RSPT_W4_TOP, bool SPH = false>
__global__ __launch_bounds__(BLOCK) RSPT_W4_ATTR void k_trace_w4(RSPT_W4_ARGS) {
    constexpr bool QUAD = false;   // (the quadric arm lives in k_trace_w4quad below: this template's parameters, and so its instantiations' names, stay as they were)
#include "trace_w4_body.h"
}

// The same walk for scenes that hold a disk or a cylinder (ABI 27): no instances, the default workgroup shape, every leaf entry with MF_SPHERE tested by its
// slot's kind.  A kernel of its own, not a ninth template parameter of k_trace_w4, so that every instantiation built before keeps its name and its figures.
#ifdef RSPT_W4_WAVES
#define RSPT_W4_ATTR_QUAD __attribute__((amdgpu_waves_per_eu(RSPT_W4_WAVES, RSPT_W4_WAVES)))
#else
#define RSPT_W4_ATTR_QUAD __attribute__((amdgpu_waves_per_eu(1, 8)))
#endif
template <bool ANY, int OUT_MODE, int ALPHA>
__global__ __launch_bounds__(RSPT_PW_BLOCK) RSPT_W4_ATTR_QUAD void k_trace_w4quad(RSPT_W4_ARGS) {
    constexpr bool INST = false, ANIM = false, SPH = true, QUAD = true;
    constexpr int BLOCK = RSPT_PW_BLOCK, TOPCAP = RSPT_W4_TOP;
#include "trace_w4_body.h"
}

}  // namespace rspt
