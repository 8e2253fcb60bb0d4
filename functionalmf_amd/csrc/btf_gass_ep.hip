// EP-centred GASS proposals (btf_gass_ep.h) and the binary row features of the constrained model
// (btf_gass_features.h): the kernels, one compilation unit of their own.  btf_abi.hip launches them through the
// function pointers below (counted under BTF_K_ESS).  gfx950 only.
#define BTF_GASS_EP_UNIT
#include "btf_gass_ep.h"
#include "btf_gass_features.h"

namespace btf {

#define GEP_CASES(F) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10)

GassEpKernel gass_ep_rows_fn(int K) {
  switch (K) {
#define GEP_R(KV) case KV: return gass_ep_rows_kernel<KV>;
    GEP_CASES(GEP_R)
#undef GEP_R
    default: return nullptr;
  }
}

GassEpKernel gass_ep_cols_fn(int K) {
  switch (K) {
#define GEP_C(KV) case KV: return gass_ep_cols_kernel<KV>;
    GEP_CASES(GEP_C)
#undef GEP_C
    default: return nullptr;
  }
}

GassEpFixKernel gass_ep_fix_fn() { return gass_ep_fix_kernel; }
GassEpCommitKernel gass_ep_commit_fn() { return gass_ep_commit_kernel; }

GassFeatRcKernel gass_feat_rc_fn() { return gass_feat_rc_kernel; }
GassFeatKernel gass_feat_analyse_fn() { return gass_feat_analyse_kernel; }
GassBernKernel gass_bern_eval_fn(bool rows, bool ep) {
  if (rows) return ep ? gass_bern_eval_kernel<true, true> : gass_bern_eval_kernel<true, false>;
  return gass_bern_eval_kernel<false, false>;      // (the feature chains' prior is N(0, I): no EP centre)
}

}  // namespace btf
