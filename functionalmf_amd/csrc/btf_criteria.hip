// Explicit instantiations of the model-selection criteria kernels (btf_criteria.h): one compilation unit of their own.
// gfx950 only.
#define BTF_CRIT_UNIT
#include "btf_criteria.h"

namespace btf {
#define BTF_D template __global__
BTF_CRIT_SET(BTF_D, 1) BTF_CRIT_SET(BTF_D, 2) BTF_CRIT_SET(BTF_D, 3) BTF_CRIT_SET(BTF_D, 4) BTF_CRIT_SET(BTF_D, 5)
BTF_CRIT_SET(BTF_D, 6) BTF_CRIT_SET(BTF_D, 7) BTF_CRIT_SET(BTF_D, 8) BTF_CRIT_SET(BTF_D, 9) BTF_CRIT_SET(BTF_D, 10)
BTF_CRIT_PLUGIN_SET(BTF_D)
#undef BTF_D
}  // namespace btf
