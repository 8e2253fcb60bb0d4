// The gamma-grid likelihood (btf_gamma_grid.h): the kernels, one compilation unit of their own.  btf_abi.hip launches
// them through the function pointers below (counted under BTF_K_ESS).  gfx950 only.
#define BTF_GAMMA_GRID_UNIT
#include "btf_gamma_grid.h"

namespace btf {

#define GG_CASES(F) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10)

GgLLKernel gg_ll_rows_fn(int K) {
  switch (K) {
#define GG_R(KV) case KV: return gg_ll_rows_kernel<KV>;
    GG_CASES(GG_R)
#undef GG_R
    default: return nullptr;
  }
}

GgLLKernel gg_ll_cols_fn(int K) {
  switch (K) {
#define GG_C(KV) case KV: return gg_ll_cols_kernel<KV>;
    GG_CASES(GG_C)
#undef GG_C
    default: return nullptr;
  }
}

GgEvalKernel gg_eval_fn(bool rows, bool ep) {
  if (rows) return ep ? gg_eval_kernel<true, true> : gg_eval_kernel<true, false>;
  return ep ? gg_eval_kernel<false, true> : gg_eval_kernel<false, false>;
}

GgLogsumKernel gg_logsum_fn() { return gg_logsum_kernel; }

}  // namespace btf
