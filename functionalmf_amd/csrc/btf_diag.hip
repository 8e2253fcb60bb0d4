// Explicit instantiations of the convergence-diagnostics kernel (btf_diag.h): one compilation unit of its own.
// gfx950 only.
#define BTF_DIAG_UNIT
#include "btf_diag.h"

namespace btf {
#define BTF_D template __global__
BTF_DIAG_SET(BTF_D)
#undef BTF_D
}  // namespace btf
