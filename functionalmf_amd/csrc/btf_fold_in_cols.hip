// Folding new columns into a fitted posterior (btf_fold_in_cols.h): the kernel, one compilation unit of its own.
// btf_analysis.hip launches it through the function pointer below (counted under BTF_K_CRITERIA).  gfx950 only.
#define BTF_FOLD_COLS_UNIT
#include "btf_fold_in_cols.h"

namespace btf {

#define FOLDC_CASES(F) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10)

FoldColsKernel fold_cols_fn(int K, int family) {
  switch (K) {
#define FOLDC_K(KV)                                                                         \
  case KV:                                                                                  \
    return family == FOLDC_GAUSSIAN ? fold_cols_kernel<KV, FOLDC_GAUSSIAN>                  \
           : family == FOLDC_BINOMIAL ? fold_cols_kernel<KV, FOLDC_BINOMIAL> : nullptr;
    FOLDC_CASES(FOLDC_K)
#undef FOLDC_K
    default: return nullptr;
  }
}

// the Negative-Binomial family (btf_negbin_fold_in_cols), through a getter of its own
FoldColsKernel fold_cols_negbin_fn(int K) {
  switch (K) {
#define FOLDC_K(KV) \
  case KV: return fold_cols_kernel<KV, FOLDC_NEGBIN>;
    FOLDC_CASES(FOLDC_K)
#undef FOLDC_K
    default: return nullptr;
  }
}

}  // namespace btf
