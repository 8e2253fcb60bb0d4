// Folding new rows into a fitted posterior (btf_fold_in.h), and into a Negative-Binomial fit with a fixed or a sampled rate
// (btf_negbin_fold_rows.h): the kernels, one compilation unit of their own.  btf_analysis.hip launches them through the
// function pointers below (counted under BTF_K_CRITERIA).  gfx950 only.
#define BTF_FOLD_UNIT
#include "btf_fold_in.h"
#include "btf_negbin_fold_rows.h"

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

NegbinFoldRowsKernel negbin_fold_rows_fn(int K, int sampled) {
  switch (K) {
#define FOLD_K(KV) \
  case KV: return sampled ? negbin_fold_rows_kernel<KV, true> : negbin_fold_rows_kernel<KV, false>;
    FOLD_CASES(FOLD_K)
#undef FOLD_K
    default: return nullptr;
  }
}

}  // namespace btf
