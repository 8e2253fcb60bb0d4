// The posterior curve functionals (btf_functionals.h) and the simultaneous bands (btf_bands.h), which share their sweep and
// sort idiom: the kernels, one compilation unit of their own.  btf_analysis.hip launches them through the function pointers
// below (counted under BTF_K_CRITERIA).  gfx950 only.
#define BTF_FUNC_UNIT
#include "btf_functionals.h"
#include "btf_bands.h"

namespace btf {

#define FUNC_CASES(F) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10)

FuncKernel func_sweep_fn(int K, int transform) {
  switch (K) {
#define FUNC_S(KV)                                                   \
  case KV:                                                           \
    return transform == 0 ? func_sweep_kernel<KV, 0> : transform == 1 ? func_sweep_kernel<KV, 1> \
           : transform == 2 ? func_sweep_kernel<KV, 2> : nullptr;
    FUNC_CASES(FUNC_S)
#undef FUNC_S
    default: return nullptr;
  }
}

// the band kernels (btf_bands.h) at the same nembeds and transforms
#define BAND_CASE(KERNEL, KV)                                        \
  case KV:                                                           \
    return transform == 0 ? KERNEL<KV, 0> : transform == 1 ? KERNEL<KV, 1> : transform == 2 ? KERNEL<KV, 2> : nullptr;
#define BAND_FN(NAME, KERNEL)                                                                                  \
  BandKernel NAME(int K, int transform) {                                                                      \
    switch (K) {                                                                                               \
      BAND_CASE(KERNEL, 1) BAND_CASE(KERNEL, 2) BAND_CASE(KERNEL, 3) BAND_CASE(KERNEL, 4) BAND_CASE(KERNEL, 5) \
      BAND_CASE(KERNEL, 6) BAND_CASE(KERNEL, 7) BAND_CASE(KERNEL, 8) BAND_CASE(KERNEL, 9) BAND_CASE(KERNEL, 10) \
      default: return nullptr;                                                                                 \
    }                                                                                                          \
  }
BAND_FN(band_moments_fn, band_moments_kernel)
BAND_FN(band_sweep_fn, band_sweep_kernel)
BAND_FN(band_rank_depth_fn, band_rank_depth_kernel)
BAND_FN(band_rank_write_fn, band_rank_write_kernel)
#undef BAND_FN
#undef BAND_CASE
BandKernel band_supt_fn() { return band_supt_kernel; }
BandKernel band_rank_k_fn() { return band_rank_k_kernel; }

FuncKernel func_sort_fn() { return func_sort_kernel; }
FuncGatherKernel func_gather_fn() { return func_gather_kernel; }

}  // namespace btf
