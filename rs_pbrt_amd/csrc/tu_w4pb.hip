// one group of kernel instantiations of librspt.so (tu_decl.h says which and why)
#include <hip/hip_runtime.h>
#include "../../include/rspt.h"
#define RSPT_TU_TEMPLATES_ONLY
#define RSPT_TU_X
#define RSPT_TU_GROUP_W4PB
#include "tu_decl.h"
#ifdef RSPT_PK_COUNT   // the timing-only counter build (trace_packet.h): {records fetched, leaves gated, bundles walked as one (packets, for the bundles handed to the packet code)} since the last call
extern "C" int rspt_pk_count_pb(unsigned long long* out3) {
    unsigned long long zero[3] = {0, 0, 0};
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out3, HIP_SYMBOL(rspt::g_pk_count), sizeof zero) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(rspt::g_pk_count), zero, sizeof zero) == hipSuccess ? 0 : -1;
}
#endif
