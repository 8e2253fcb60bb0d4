// Explicit instantiations of the PSIS-LOO kernels (btf_loo.h): one compilation unit of their own.
// gfx950 only.
#define BTF_LOO_UNIT
#include "btf_loo.h"

namespace btf {
#define BTF_D template __global__
BTF_LOO_SET(BTF_D)
#undef BTF_D
}  // namespace btf
