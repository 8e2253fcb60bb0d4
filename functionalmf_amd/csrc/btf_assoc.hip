// The posterior feature association (btf_assoc.h): the kernels, one compilation unit of their own.  btf_analysis.hip launches
// them through the function pointers below (counted under BTF_K_CRITERIA).  gfx950 only.
#define BTF_ASSOC_UNIT
#include "btf_assoc.h"

namespace btf {

#define ASSOC_CASES(F) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10)
#define ASSOC_FN(NAME, KERNEL)                 \
  AssocKernel NAME(int K) {                    \
    switch (K) {                               \
      ASSOC_CASES(ASSOC_CASE_##KERNEL)         \
      default: return nullptr;                 \
    }                                          \
  }
#define ASSOC_CASE_moments(KV) case KV: return assoc_moments_kernel<KV>;
#define ASSOC_CASE_reduce(KV) case KV: return assoc_reduce_kernel<KV>;
#define ASSOC_CASE_values(KV) case KV: return assoc_values_kernel<KV>;
#define ASSOC_CASE_pbar(KV) case KV: return assoc_pbar_kernel<KV>;

ASSOC_FN(assoc_moments_fn, moments)
ASSOC_FN(assoc_reduce_fn, reduce)
ASSOC_FN(assoc_values_fn, values)
ASSOC_FN(assoc_pbar_fn, pbar)

AssocKernel assoc_gbar_fn() { return assoc_gbar_kernel; }
AssocKernel assoc_gbar_finish_fn() { return assoc_gbar_finish_kernel; }
AssocKernel assoc_cross_fn() { return assoc_cross_kernel; }

}  // namespace btf
