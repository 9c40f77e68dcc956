// Which kernel instantiations live in which translation unit.  librspt.so is built from several .hip files compiled side by side
// (one hipcc run over everything took eight minutes): librspt.hip holds the host code and the small kernels and sees the heavy
// templates below only as `extern template` declarations (RSPT_TU_X = extern, RSPT_TU_ALL); tu.hip defines RSPT_TU_X empty, is compiled
// once per group with one RSPT_TU_GROUP_* on the command line (csrc/Makefile GROUPS) and so carries the device code and the launch stubs of that group.
// Every kernel's parameter list is the macro next to its definition (RSPT_W4_ARGS, RSPT_SHADE_ARGS, ...).
#pragma once
#include "tile_serial.h"
#include "lane_serial.h"
#include "trace_w4.h"
#include "trace_w4q.h"
#include "trace_packet.h"
#include "trace_frustum.h"
#include "trace_bundle.h"

namespace rspt {

// ---- the shade stage's feature sets (kernels.h k_shade<F>; librspt.hip g_shade_variants) ----
constexpr uint32_t SV_DIFFUSE = RSPT_SF_LOBE(RSPT_BXDF_LAMBERT_R) | SF_L_AREA | SF_SOBOL;           // matte scenes under area lights: C1, C2
constexpr uint32_t SV_PLASTIC = SV_DIFFUSE | RSPT_SF_LOBE(RSPT_BXDF_MICROFACET_R) | SF_VERTEX;      // + plastic, smooth-shaded meshes: the C3 stand-in
constexpr uint32_t SV_TEXTURED = SV_PLASTIC | RSPT_SF_LOBE(RSPT_BXDF_OREN_NAYAR) | SF_TEX;          // + textured materials: the C4 stand-in
constexpr uint32_t SV_GENERIC = SF_ALL & ~SF_DYNAMIC & ~SF_ANIM;
// the same three under the Halton sampler (the reference's default, api.rs:526): without them a Halton render took the generic instantiation
// (212 VGPRs = 2 waves: C2 403 against Sobol's 473 M samples/s, the C3 stand-in 1705 against 2018)
constexpr uint32_t SV_DIFFUSE_H = (SV_DIFFUSE & ~SF_SOBOL) | SF_HALTON, SV_PLASTIC_H = (SV_PLASTIC & ~SF_SOBOL) | SF_HALTON, SV_TEXTURED_H = (SV_TEXTURED & ~SF_SOBOL) | SF_HALTON;
constexpr uint32_t SV_DYNAMIC = SF_ALL & ~SF_ANIM;                                                  // + per-hit lobe lists; SF_ALL itself: + moving instances
// scenes with analytic spheres (dev_bsdf.h shade_sph): the generic and the dynamic set with the sphere arm; the sets above keep SF_TRIS_ONLY and so their code
constexpr uint32_t SV_GENERIC_SPH = SV_GENERIC & ~SF_TRIS_ONLY, SV_DYNAMIC_SPH = SV_DYNAMIC & ~SF_TRIS_ONLY;
// scenes with a projection or goniometric light (ABI 24; dev_bsdf.h shade_ml): the generic set and the all-features set with those two arms; every set above
// keeps SF_NO_MAPLIGHT (or never had SF_L_MAP) and so its code
// scenes with a disk or a cylinder (ABI 27; dev_bsdf.h shade_quad): the two sphere sets with the quadric arm in place of the sphere arm; every set above keeps
// SF_NO_QUADRIC and so its code
constexpr uint32_t SV_GENERIC_QUAD = SV_GENERIC_SPH & ~SF_NO_QUADRIC, SV_DYNAMIC_QUAD = SV_DYNAMIC_SPH & ~SF_NO_QUADRIC;
constexpr uint32_t SV_GENERIC_ML = SV_GENERIC & ~SF_NO_MAPLIGHT, SV_ALL_ML = SF_ALL & ~SF_NO_MAPLIGHT;

#define RSPT_TU_TS(I, A, M) RSPT_TU_X template __global__ void k_tile_serial<I, A, M>(RSPT_TS_ARGS);
#define RSPT_TU_TS2(I, M) RSPT_TU_TS(I, false, M) RSPT_TU_TS(I, true, M)
// the shade kernels: X is empty for the exact builds and _fast for the fast-math ones (kernels.h k_shade*, k_shade_fast*)
#define RSPT_TU_SHADE(X, F) RSPT_TU_X template __global__ void k_shade##X<F>(RSPT_SHADE_ARGS);
#define RSPT_TU_SHADE_W(X, F, W) RSPT_TU_X template __global__ void k_shade##X##_w<F, W>(RSPT_SHADE_ARGS);
#define RSPT_TU_SHADE_M(X, F) RSPT_TU_X template __global__ void k_shade##X##_m<F>(RSPT_SHADE_ARGS);          /* the MOVE forms (kernels.h PathBuf::move): one per feature set, */
#define RSPT_TU_SHADE_MW(X, F, W) RSPT_TU_X template __global__ void k_shade##X##_mw<F, W>(RSPT_SHADE_ARGS);  /* built the way that set's default is built */
#define RSPT_TU_W4(ANY, OM, I, A) RSPT_TU_X template __global__ void k_trace_w4<ANY, OM, I, A>(RSPT_W4_ARGS);
#define RSPT_TU_W4A1(ANY, OM, A) RSPT_TU_X template __global__ void k_trace_w4<ANY, OM, true, A, true>(RSPT_W4_ARGS);
#define RSPT_TU_W4AF(ANY, OM, A) RSPT_TU_X template __global__ void k_trace_fixup<ANY, OM, true, A, true>(RSPT_FIXUP_ARGS);
#define RSPT_TU_W4A(ANY, OM) RSPT_TU_W4A1(ANY, OM, 0) RSPT_TU_W4AF(ANY, OM, false)   /* moving instances */
#define RSPT_TU_W4AM(ANY, OM) RSPT_TU_W4A1(ANY, OM, 1) RSPT_TU_W4A1(ANY, OM, 2) RSPT_TU_W4AF(ANY, OM, true)   /* moving instances next to alpha-masked meshes */
#define RSPT_TU_W4B(ANY, OM, B, T) RSPT_TU_X template __global__ void k_trace_w4<ANY, OM, false, 0, false, B, T>(RSPT_W4_ARGS);   /* big workgroups, big LDS top */
#define RSPT_TU_W4SPH(ANY, A) RSPT_TU_W4SPHO(ANY, 1, A)
#define RSPT_TU_W4SPHO(ANY, OM, A) /* scenes with spheres: the trace hook (OM 1), the render's queues (OM 0) */ \
    RSPT_TU_X template __global__ void k_trace_w4<ANY, OM, false, A, false, RSPT_PW_BLOCK, RSPT_W4_TOP, true>(RSPT_W4_ARGS);
#define RSPT_TU_W4QUAD(ANY, OM, A) /* scenes with a disk or a cylinder (ABI 27): the trace hook (OM 1), the render's queues (OM 0) */ \
    RSPT_TU_X template __global__ void k_trace_w4quad<ANY, OM, A>(RSPT_W4_ARGS);
#define RSPT_TU_W4_4(ANY, OM) RSPT_TU_W4(ANY, OM, false, 0) RSPT_TU_W4(ANY, OM, false, 1) RSPT_TU_W4(ANY, OM, true, 0) RSPT_TU_W4(ANY, OM, true, 1)
#define RSPT_TU_W4_S(ANY, OM) RSPT_TU_W4(ANY, OM, false, 2) RSPT_TU_W4(ANY, OM, true, 2)   /* alpha masks evaluated in line (alpha_simple) */
#define RSPT_TU_REF(ANY, OM, C, I, A) RSPT_TU_X template __global__ void k_trace<ANY, OM, C, I, A>(RSPT_TRACE_ARGS);
#define RSPT_TU_REFA1(ANY, OM, A) RSPT_TU_X template __global__ void k_trace<ANY, OM, false, true, A, true>(RSPT_TRACE_ARGS);   /* moving instances (traverse<.., ANIM>) */
#define RSPT_TU_REFA(ANY, OM) RSPT_TU_REFA1(ANY, OM, false) RSPT_TU_REFA1(ANY, OM, true)   /* ... alone and next to alpha-masked meshes */
#define RSPT_TU_REF8(ANY, OM) \
    RSPT_TU_REF(ANY, OM, false, false, false) RSPT_TU_REF(ANY, OM, false, false, true) RSPT_TU_REF(ANY, OM, false, true, false) RSPT_TU_REF(ANY, OM, false, true, true) \
    RSPT_TU_REF(ANY, OM, true, false, false) RSPT_TU_REF(ANY, OM, true, false, true) RSPT_TU_REF(ANY, OM, true, true, false) RSPT_TU_REF(ANY, OM, true, true, true)
#define RSPT_TU_FIX(ANY, OM, I, A) RSPT_TU_X template __global__ void k_trace_fixup<ANY, OM, I, A>(RSPT_FIXUP_ARGS);
#define RSPT_TU_FIX4(ANY, OM) RSPT_TU_FIX(ANY, OM, false, false) RSPT_TU_FIX(ANY, OM, false, true) RSPT_TU_FIX(ANY, OM, true, false) RSPT_TU_FIX(ANY, OM, true, true)

#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS0A)
RSPT_TU_TS2(false, 0)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS0B)
RSPT_TU_TS2(true, 0)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS1A)
RSPT_TU_TS2(false, 1)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS1B)
RSPT_TU_TS2(true, 1)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS2A)
RSPT_TU_TS2(false, 2)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS2B)
RSPT_TU_TS2(true, 2)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS3A)
RSPT_TU_TS2(false, 3)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS3B)
RSPT_TU_TS2(true, 3)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS4A)
RSPT_TU_TS2(false, 4)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS4B)
RSPT_TU_TS2(true, 4)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS5)
RSPT_TU_TS2(true, 5)   /* path / ao under the pixel samplers over moving instances */
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS6)
RSPT_TU_TS2(true, 6)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS7)
RSPT_TU_TS2(true, 7)   /* volpath / directlighting per tile over moving instances */
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS8)
RSPT_TU_TS2(true, 8)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS9A)
RSPT_TU_TS2(false, 9)   /* whitted per tile */
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS9B)
RSPT_TU_TS2(true, 9)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_TS10)
RSPT_TU_TS2(true, 10)   /* whitted per tile over moving instances */
#endif
#define RSPT_TU_LANE(I, A) RSPT_TU_X template __global__ void k_lane_dl<I, A>(RSPT_LANE_ARGS);
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_LANE_A)
RSPT_TU_LANE(false, false) RSPT_TU_LANE(false, true)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_LANE_B)
RSPT_TU_LANE(true, false) RSPT_TU_LANE(true, true)
#endif
#define RSPT_TU_LANE_ANIM(A) RSPT_TU_X template __global__ void k_lane_dl<true, A, true>(RSPT_LANE_ARGS);
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_LANE_C)
RSPT_TU_LANE_ANIM(false) RSPT_TU_LANE_ANIM(true)   /* the per-lane directlighting over moving instances */
#endif
#define RSPT_TU_LANE_WH(I, A, M) RSPT_TU_X template __global__ void k_lane_dl<I, A, M, true>(RSPT_LANE_ARGS);
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_LANE_WA)
RSPT_TU_LANE_WH(false, false, false) RSPT_TU_LANE_WH(false, true, false)   /* whitted, one lane per camera sample */
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_LANE_WB)
RSPT_TU_LANE_WH(true, false, false) RSPT_TU_LANE_WH(true, true, false)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_LANE_WC)
RSPT_TU_LANE_WH(true, false, true) RSPT_TU_LANE_WH(true, true, true)
#endif
// ---- the shade groups.  The lists that the exact builds (X empty) share with their fast-math twins (X = _fast: kernels.h k_shade_fast*; rspt_set_shade_math,
// DESIGN section 5.3a).  A fast group is compiled with RSPT_FAST_MATH defined and, but for the generic set's two, without correctly rounded f32 division /
// square root (csrc/Makefile FAST_GROUPS).  The dynamic, moving, sphere, sphere-light, quadric and map-light sets have no fast build.
#define RSPT_TU_LIST_A(X) \
    RSPT_TU_SHADE(X, SV_DIFFUSE) RSPT_TU_SHADE_W(X, SV_DIFFUSE, 3) RSPT_TU_SHADE_W(X, SV_DIFFUSE, 4) RSPT_TU_SHADE(X, SV_PLASTIC) RSPT_TU_SHADE_W(X, SV_PLASTIC, 3) RSPT_TU_SHADE_W(X, SV_PLASTIC, 4)
#define RSPT_TU_LIST_B(X) RSPT_TU_SHADE(X, SV_TEXTURED) RSPT_TU_SHADE_W(X, SV_TEXTURED, 3) RSPT_TU_SHADE_W(X, SV_TEXTURED, 4)
#define RSPT_TU_LIST_GENERIC(X) RSPT_TU_SHADE(X, SV_GENERIC) RSPT_TU_SHADE_W(X, SV_GENERIC, 3) RSPT_TU_SHADE_W(X, SV_GENERIC, 4)
#define RSPT_TU_LIST_H(X) \
    RSPT_TU_SHADE(X, SV_DIFFUSE_H) RSPT_TU_SHADE_W(X, SV_DIFFUSE_H, 3) RSPT_TU_SHADE(X, SV_PLASTIC_H) RSPT_TU_SHADE_W(X, SV_PLASTIC_H, 3) RSPT_TU_SHADE(X, SV_TEXTURED_H) RSPT_TU_SHADE_W(X, SV_TEXTURED_H, 3)
#define RSPT_TU_LIST_MA(X) RSPT_TU_SHADE_MW(X, SV_DIFFUSE, 3) RSPT_TU_SHADE_MW(X, SV_PLASTIC, 3) RSPT_TU_SHADE_M(X, SV_DIFFUSE) RSPT_TU_SHADE_M(X, SV_PLASTIC)
#define RSPT_TU_LIST_MB(X) RSPT_TU_SHADE_M(X, SV_TEXTURED) RSPT_TU_SHADE_MW(X, SV_TEXTURED_H, 3)
#define RSPT_TU_LIST_MC(X) RSPT_TU_SHADE_M(X, SV_GENERIC)
#define RSPT_TU_LIST_MH(X) RSPT_TU_SHADE_MW(X, SV_DIFFUSE_H, 3) RSPT_TU_SHADE_MW(X, SV_PLASTIC_H, 3)
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_A)
RSPT_TU_LIST_A()
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_FA)
RSPT_TU_LIST_A(_fast)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_B)
RSPT_TU_LIST_B()
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_FB)
RSPT_TU_LIST_B(_fast)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_C)
RSPT_TU_LIST_GENERIC() RSPT_TU_SHADE(, SV_DYNAMIC) RSPT_TU_SHADE(, SF_ALL)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_FC)
RSPT_TU_LIST_GENERIC(_fast)   /* the generic set only */
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_H)
RSPT_TU_LIST_H()
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_FH)
RSPT_TU_LIST_H(_fast)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_MA)
RSPT_TU_LIST_MA()
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_FMA)
RSPT_TU_LIST_MA(_fast)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_MB)
RSPT_TU_LIST_MB()
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_FMB)
RSPT_TU_LIST_MB(_fast)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_MC)
RSPT_TU_LIST_MC()
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_FMC)
RSPT_TU_LIST_MC(_fast)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_MH)
RSPT_TU_LIST_MH()
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_FMH)
RSPT_TU_LIST_MH(_fast)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_S)
RSPT_TU_SHADE(, SV_GENERIC_SPH) RSPT_TU_SHADE(, SV_DYNAMIC_SPH)   /* scenes with spheres; no MOVE form: they keep slots for life */
#endif
// scenes with spheres that hold a sphere area light, served while the sphere-light gate is on (rspt_set_sphere_lights): the two sphere sets with the
// sphere-light arms of shade_path (kernels.h k_shade_sl); every kernel above keeps its name and its code
#define RSPT_TU_SHADE_SL(F) RSPT_TU_X template __global__ void k_shade_sl<F>(RSPT_SHADE_ARGS);
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_SL)
RSPT_TU_SHADE_SL(SV_GENERIC_SPH)   /* no MOVE form, no fast-math form */
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_SLD)
RSPT_TU_SHADE_SL(SV_DYNAMIC_SPH)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_Q)
RSPT_TU_SHADE(, SV_GENERIC_QUAD)   /* scenes with a disk or a cylinder; no MOVE form, as for spheres */
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_QD)
RSPT_TU_SHADE(, SV_DYNAMIC_QUAD)
#endif
// scenes with a disk or a cylinder that hold an area light on a quadric, served while the quadric-light gate is on (rspt_set_quadric_lights): the two quadric
// sets with the quadric-light arms of shade_path (kernels.h k_shade_ql); every kernel above keeps its name and its code
#define RSPT_TU_SHADE_QL(F) RSPT_TU_X template __global__ void k_shade_ql<F>(RSPT_SHADE_ARGS);
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_QL)
RSPT_TU_SHADE_QL(SV_GENERIC_QUAD)   /* no MOVE form, no fast-math form */
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_QLD)
RSPT_TU_SHADE_QL(SV_DYNAMIC_QUAD)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_SHADE_L)
RSPT_TU_SHADE(, SV_GENERIC_ML) RSPT_TU_SHADE(, SV_ALL_ML)   /* scenes with projection / goniometric lights; no MOVE form */
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_W4Q)
RSPT_TU_X template __global__ void k_trace_w4q<0>(RSPT_W4Q_ARGS);
RSPT_TU_X template __global__ void k_trace_w4q<1>(RSPT_W4Q_ARGS);
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_W4PK)
#define RSPT_TU_W4PK(OM) RSPT_TU_X template __global__ void k_trace_w4pk<OM>(RSPT_PK_ARGS);
RSPT_TU_W4PK(0) RSPT_TU_W4PK(1)   /* the packet walk of coherent closest-hit launches (trace_packet.h): the render's queues, the trace hook */
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_W4PF)
#define RSPT_TU_W4PF(OM) RSPT_TU_X template __global__ void k_trace_w4pf<OM>(RSPT_PK_ARGS);
RSPT_TU_W4PF(0) RSPT_TU_W4PF(1)   /* the packet walk with one frustum test per record (trace_frustum.h): the render's queues, the trace hook */
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_W4PB)
#define RSPT_TU_W4PB(OM, R) RSPT_TU_X template __global__ void k_trace_w4pb<OM, R>(RSPT_PK_ARGS);
RSPT_TU_W4PB(0, 2) RSPT_TU_W4PB(1, 2) RSPT_TU_W4PB(0, 4) RSPT_TU_W4PB(1, 4)   /* the frustum walk for bundles of two / four packets per wave (trace_bundle.h) */
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_W4)
RSPT_TU_W4_4(false, 0) RSPT_TU_W4_4(false, 1) RSPT_TU_W4_4(true, 0) RSPT_TU_W4_4(true, 1)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_W4S)
RSPT_TU_W4_S(false, 0) RSPT_TU_W4_S(false, 1) RSPT_TU_W4_S(true, 0) RSPT_TU_W4_S(true, 1)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_W4SPH)
RSPT_TU_W4SPH(false, 0) RSPT_TU_W4SPH(false, 1) RSPT_TU_W4SPH(false, 2) RSPT_TU_W4SPH(true, 0) RSPT_TU_W4SPH(true, 1) RSPT_TU_W4SPH(true, 2)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_W4SPH0)
RSPT_TU_W4SPHO(false, 0, 0) RSPT_TU_W4SPHO(false, 0, 1) RSPT_TU_W4SPHO(false, 0, 2) RSPT_TU_W4SPHO(true, 0, 0) RSPT_TU_W4SPHO(true, 0, 1) RSPT_TU_W4SPHO(true, 0, 2)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_W4QUAD)
RSPT_TU_W4QUAD(false, 1, 0) RSPT_TU_W4QUAD(false, 1, 1) RSPT_TU_W4QUAD(false, 1, 2) RSPT_TU_W4QUAD(true, 1, 0) RSPT_TU_W4QUAD(true, 1, 1) RSPT_TU_W4QUAD(true, 1, 2)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_W4QUAD0)
RSPT_TU_W4QUAD(false, 0, 0) RSPT_TU_W4QUAD(false, 0, 1) RSPT_TU_W4QUAD(false, 0, 2) RSPT_TU_W4QUAD(true, 0, 0) RSPT_TU_W4QUAD(true, 0, 1) RSPT_TU_W4QUAD(true, 0, 2)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_W4A)
RSPT_TU_W4A(false, 0) RSPT_TU_W4A(false, 1) RSPT_TU_W4A(true, 0) RSPT_TU_W4A(true, 1)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_W4AM)
RSPT_TU_W4AM(false, 0) RSPT_TU_W4AM(false, 1) RSPT_TU_W4AM(true, 0) RSPT_TU_W4AM(true, 1)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_W4B)
RSPT_TU_W4B(false, 0, 1024, 512) RSPT_TU_W4B(false, 1, 1024, 512) RSPT_TU_W4B(true, 0, 1024, 512) RSPT_TU_W4B(true, 1, 1024, 512)
RSPT_TU_W4B(false, 0, 512, 256) RSPT_TU_W4B(false, 1, 512, 256) RSPT_TU_W4B(true, 0, 512, 256) RSPT_TU_W4B(true, 1, 512, 256)
#endif
#if defined(RSPT_TU_ALL) || defined(RSPT_TU_GROUP_REF)
RSPT_TU_REF8(false, 0) RSPT_TU_REF8(false, 1) RSPT_TU_REF8(true, 0) RSPT_TU_REF8(true, 1)
RSPT_TU_FIX4(false, 0) RSPT_TU_FIX4(false, 1) RSPT_TU_FIX4(true, 0) RSPT_TU_FIX4(true, 1)
RSPT_TU_REFA(false, 0) RSPT_TU_REFA(false, 1) RSPT_TU_REFA(true, 0) RSPT_TU_REFA(true, 1)
#endif

}  // namespace rspt
