// Folding new rows into a fitted posterior (btf_fold_in.h): the kernel, one compilation unit of its own.  btf_analysis.hip
// launches it through the function pointer below (counted under BTF_K_CRITERIA).  gfx950 only.
#define BTF_FOLD_UNIT
#include "btf_fold_in.h"

namespace btf {

#define FOLD_CASES(F) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10)

FoldKernel fold_in_fn(int K, int family) {
  switch (K) {
#define FOLD_K(KV)                                                                          \
  case KV:                                                                                  \
    return family == FOLD_GAUSSIAN ? fold_in_kernel<KV, FOLD_GAUSSIAN>                      \
           : family == FOLD_BINOMIAL ? fold_in_kernel<KV, FOLD_BINOMIAL> : nullptr;
    FOLD_CASES(FOLD_K)
#undef FOLD_K
    default: return nullptr;
  }
}

}  // namespace btf
