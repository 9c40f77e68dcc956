// one group of fast-math shade instantiations of librspt.so (tu_decl.h says which): RSPT_FAST_MATH before every include, and the Makefile
// compiles this unit without correctly rounded f32 division / square root (FAST_FLAGS)
#define RSPT_FAST_MATH
#include <hip/hip_runtime.h>
#include "../../include/rspt.h"
#define RSPT_TU_TEMPLATES_ONLY
#define RSPT_TU_X
#define RSPT_TU_GROUP_SHADE_FMA
#include "tu_decl.h"
