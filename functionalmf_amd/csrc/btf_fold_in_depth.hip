// Folding new depth slices into a fitted posterior (btf_fold_in_depth.h): the kernel, one compilation unit of its own.
// btf_analysis.hip launches it through the function pointer below (counted under BTF_K_CRITERIA).  gfx950 only.
#define BTF_FOLD_DEPTH_UNIT
#include "btf_fold_in_depth.h"

namespace btf {

#define FOLDD_CASES(F) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10)

FoldDepthKernel fold_depth_fn(int K, int family) {
  switch (K) {
#define FOLDD_K(KV)                                                                         \
  case KV:                                                                                  \
    return family == FOLDD_GAUSSIAN ? fold_depth_kernel<KV, FOLDD_GAUSSIAN>                 \
           : family == FOLDD_BINOMIAL ? fold_depth_kernel<KV, FOLDD_BINOMIAL> : nullptr;
    FOLDD_CASES(FOLDD_K)
#undef FOLDD_K
    default: return nullptr;
  }
}

// the Negative-Binomial family (btf_negbin_fold_in_depth), through a getter of its own
FoldDepthKernel fold_depth_negbin_fn(int K) {
  switch (K) {
#define FOLDD_K(KV) \
  case KV: return fold_depth_kernel<KV, FOLDD_NEGBIN>;
    FOLDD_CASES(FOLDD_K)
#undef FOLDD_K
    default: return nullptr;
  }
}

}  // namespace btf
