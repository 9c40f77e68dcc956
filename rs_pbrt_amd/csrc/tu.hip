// One group of kernel instantiations of librspt.so: compiled once per group with -DRSPT_TU_GROUP_<NAME> (csrc/Makefile GROUPS; tu_decl.h says which
// instantiations a group holds and why).  The fast-math shade groups also get -DRSPT_FAST_MATH from the Makefile, so it is defined before every include.
#include <hip/hip_runtime.h>
#include "../../include/rspt.h"
#define RSPT_TU_TEMPLATES_ONLY
#define RSPT_TU_X
#include "tu_decl.h"

// ---- the hooks of the timing-only counter builds: each in the group whose kernels count, so a counter build defines each once ----
#if defined(RSPT_W4Q_COUNT) && defined(RSPT_TU_GROUP_W4Q)   // trace_w4q.h: the eight lane-occupancy counters since the last call
extern "C" int rspt_w4q_count(unsigned long long* out8) {
    unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out8, HIP_SYMBOL(rspt::g_w4q_count), sizeof zero) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(rspt::g_w4q_count), zero, sizeof zero) == hipSuccess ? 0 : -1;
}
#endif
// trace_packet.h: {records fetched, leaves tested on a pop or a gate, packets walked} since the last call; for W4PB {records fetched, leaves gated,
// bundles walked as one (packets, for the bundles handed to the packet code)}.  g_pk_count is each unit's own.
#ifdef RSPT_PK_COUNT
#define RSPT_PK_COUNT_HOOK(NAME)                                                                                                                   \
    extern "C" int NAME(unsigned long long* out3) {                                                                                                \
        unsigned long long zero[3] = {0, 0, 0};                                                                                                    \
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out3, HIP_SYMBOL(rspt::g_pk_count), sizeof zero) != hipSuccess) return -1; \
        return hipMemcpyToSymbol(HIP_SYMBOL(rspt::g_pk_count), zero, sizeof zero) == hipSuccess ? 0 : -1;                                          \
    }
#if defined(RSPT_TU_GROUP_W4PK)
RSPT_PK_COUNT_HOOK(rspt_pk_count_pk)
#elif defined(RSPT_TU_GROUP_W4PF)
RSPT_PK_COUNT_HOOK(rspt_pk_count_pf)
#elif defined(RSPT_TU_GROUP_W4PB)
RSPT_PK_COUNT_HOOK(rspt_pk_count_pb)
#endif
#endif
