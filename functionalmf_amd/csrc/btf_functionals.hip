// The posterior curve functionals (btf_functionals.h): the kernels, one compilation unit of their own.  btf_analysis.hip
// launches them through the function pointers below (counted under BTF_K_CRITERIA).  gfx950 only.
#define BTF_FUNC_UNIT
#include "btf_functionals.h"

namespace btf {

#define FUNC_CASES(F) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10)

FuncKernel func_sweep_fn(int K, int transform) {
  switch (K) {
#define FUNC_S(KV)                                                   \
  case KV:                                                           \
    return transform == 0 ? func_sweep_kernel<KV, 0> : transform == 1 ? func_sweep_kernel<KV, 1> \
           : transform == 2 ? func_sweep_kernel<KV, 2> : nullptr;
    FUNC_CASES(FUNC_S)
#undef FUNC_S
    default: return nullptr;
  }
}

FuncKernel func_sort_fn() { return func_sort_kernel; }
FuncGatherKernel func_gather_fn() { return func_gather_kernel; }

}  // namespace btf
