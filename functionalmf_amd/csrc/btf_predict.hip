// Explicit instantiations of the posterior-predictive kernels (btf_predict.h) and of the predictive-check kernel
// (btf_checks.h), which draws from the same samplers: one compilation unit of their own.  gfx950 only.
#define BTF_PRED_UNIT
#include "btf_predict.h"
#include "btf_checks.h"

namespace btf {
#define BTF_D template __global__
BTF_PRED_SET(BTF_D, 0) BTF_PRED_SET(BTF_D, 1) BTF_PRED_SET(BTF_D, 2) BTF_PRED_SET(BTF_D, 3) BTF_PRED_SET(BTF_D, 4)
BTF_CHK_SET(BTF_D, 0) BTF_CHK_SET(BTF_D, 1) BTF_CHK_SET(BTF_D, 2) BTF_CHK_SET(BTF_D, 3) BTF_CHK_SET(BTF_D, 4)
#undef BTF_D
}  // namespace btf
