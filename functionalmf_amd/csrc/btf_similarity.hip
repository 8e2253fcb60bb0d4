// The posterior similarity (btf_similarity.h): the kernels, one compilation unit of their own.  btf_analysis.hip launches
// them through the function pointers below (counted under BTF_K_CRITERIA).  gfx950 only.
#define BTF_SIM_UNIT
#include "btf_similarity.h"

namespace btf {

#define SIM_CASES(F) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10)

SimKernel sim_metric_fn(int K) {
  switch (K) {
#define SIM_M(KV) case KV: return sim_metric_kernel<KV>;
    SIM_CASES(SIM_M)
#undef SIM_M
    default: return nullptr;
  }
}

SimKernel sim_dist_fn(int K, bool cosine) {
  switch (K) {
#define SIM_D(KV) case KV: return cosine ? sim_dist_kernel<KV, true> : sim_dist_kernel<KV, false>;
    SIM_CASES(SIM_D)
#undef SIM_D
    default: return nullptr;
  }
}

SimKernel sim_root_fn() { return sim_root_kernel; }
SimKernel sim_pairs_fn() { return sim_pairs_kernel; }
SimKernel sim_finish_fn() { return sim_finish_kernel; }

}  // namespace btf
