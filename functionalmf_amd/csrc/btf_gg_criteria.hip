// The gamma-grid criteria kernels (btf_gg_criteria.h): one compilation unit of their own.  btf_analysis.hip launches them
// through the function pointers below (counted under BTF_K_CRITERIA).  gfx950 only.
#define BTF_GG_CRIT_UNIT
#include "btf_gg_criteria.h"

namespace btf {

GgCritKernel gg_crit_fn(int K) {
  switch (K) {
#define GGC_CASE(KV) case KV: return gg_crit_kernel<KV>;
    GGC_CASE(1) GGC_CASE(2) GGC_CASE(3) GGC_CASE(4) GGC_CASE(5) GGC_CASE(6) GGC_CASE(7) GGC_CASE(8) GGC_CASE(9) GGC_CASE(10)
#undef GGC_CASE
    default: return nullptr;
  }
}

GgCritKernel gg_crit_plugin_fn() { return gg_crit_plugin_kernel; }

}  // namespace btf
