// Explicit instantiations of the posterior-predictive kernels (btf_predict.h): one compilation unit of their own.
// gfx950 only.
#define BTF_PRED_UNIT
#include "btf_predict.h"

namespace btf {
#define BTF_D template __global__
BTF_PRED_SET(BTF_D, 0) BTF_PRED_SET(BTF_D, 1) BTF_PRED_SET(BTF_D, 2) BTF_PRED_SET(BTF_D, 3) BTF_PRED_SET(BTF_D, 4)
#undef BTF_D
}  // namespace btf
