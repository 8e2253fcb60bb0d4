// The Negative-Binomial criteria kernels (btf_nb_criteria.h): one compilation unit of their own.  btf_analysis.hip launches
// them through the function pointers below (counted under BTF_K_CRITERIA).  gfx950 only.
#define BTF_NB_CRIT_UNIT
#include "btf_nb_criteria.h"

namespace btf {

NbConstKernel nb_crit_const_fn(bool rows) { return rows ? nb_crit_const_kernel<true> : nb_crit_const_kernel<false>; }

NbConstKernel nb_crit_const_tab_fn() { return nb_crit_const_tab_kernel<NBC_TSB>; }

NbCritKernel nb_crit_fn(int K, bool rows) {
  switch (K) {
#define NBC_CASE(KV) case KV: return rows ? nb_crit_kernel<KV, true> : nb_crit_kernel<KV, false>;
    NBC_CASE(1) NBC_CASE(2) NBC_CASE(3) NBC_CASE(4) NBC_CASE(5) NBC_CASE(6) NBC_CASE(7) NBC_CASE(8) NBC_CASE(9) NBC_CASE(10)
#undef NBC_CASE
    default: return nullptr;
  }
}

NbCritKernel nb_crit_plugin_fn(bool rows) { return rows ? nb_crit_plugin_kernel<true> : nb_crit_plugin_kernel<false>; }

}  // namespace btf
