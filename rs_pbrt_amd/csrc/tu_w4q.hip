// one group of kernel instantiations of librspt.so (tu_decl.h says which and why)
#include <hip/hip_runtime.h>
#include "../../include/rspt.h"
#define RSPT_TU_TEMPLATES_ONLY
#define RSPT_TU_X
#define RSPT_TU_GROUP_W4Q
#include "tu_decl.h"
#ifdef RSPT_W4Q_COUNT   // the timing-only counter build (trace_w4q.h): the eight lane-occupancy counters since the last call
extern "C" int rspt_w4q_count(unsigned long long* out8) {
    unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out8, HIP_SYMBOL(rspt::g_w4q_count), sizeof zero) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(rspt::g_w4q_count), zero, sizeof zero) == hipSuccess ? 0 : -1;
}
#endif
