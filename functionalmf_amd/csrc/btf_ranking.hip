// The posterior ranking (btf_ranking.h): the kernels, one compilation unit of their own.  btf_analysis.hip launches them
// through the function pointers below (counted under BTF_K_CRITERIA).  gfx950 only.
#define BTF_RANK_UNIT
#include "btf_ranking.h"

namespace btf {

RankKernel rank_fn(bool descending) { return descending ? rank_kernel<false> : rank_kernel<true>; }
RankKernel rank_pairs_fn() { return rank_pairs_kernel; }
RankKernel rank_finish_fn() { return rank_finish_kernel; }

}  // namespace btf
