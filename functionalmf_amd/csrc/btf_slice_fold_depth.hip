// Folding new depth slices into a slice-sampled fit (btf_slice_fold_depth.h): the kernels, one compilation unit of their own.
// btf_analysis.hip launches them through the function pointer below (counted under BTF_K_CRITERIA).  gfx950 only.
#define BTF_SLICE_FOLD_DEPTH_UNIT
#include "btf_gamma_grid.h"     // (first: with the unit's macro it brings btf_ess.h, btf_kernels.h and the cell term)
#include "btf_slice_fold_depth.h"

namespace btf {

#define SFD_CASES(F) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10)

SliceFoldDepthKernel slice_fold_depth_fn(int K, int family) {
  const int link = family >= 0 && family < ESS_FAM_COUNT ? ess_link_of(family) : -1;
  switch (K) {
#define SFD_K(KV)                                                                                       \
  case KV:                                                                                              \
    return link == ESS_LINK_LOG ? slice_fold_depth_kernel<KV, ESS_LINK_LOG>                             \
           : link == ESS_LINK_IDENTITY ? slice_fold_depth_kernel<KV, ESS_LINK_IDENTITY>                 \
           : link == ESS_LINK_GENERIC ? slice_fold_depth_kernel<KV, ESS_LINK_GENERIC>                   \
           : link == ESS_LINK_GAMMA_GRID ? slice_fold_depth_kernel<KV, ESS_LINK_GAMMA_GRID> : nullptr;
    SFD_CASES(SFD_K)
#undef SFD_K
    default: return nullptr;
  }
}

}  // namespace btf
