// The monotone projection of the posterior (btf_monotone.h): the kernel, one compilation unit of its own.  btf_analysis.hip
// launches it through the function pointer below (counted under BTF_K_CRITERIA).  gfx950 only.
#define BTF_MONOTONE_UNIT
#include "btf_monotone.h"

namespace btf {

MonoKernel mono_project_fn(int K) {
  switch (K) {
#define MONO_CASE(KV) case KV: return mono_project_kernel<KV>;
    MONO_CASE(1) MONO_CASE(2) MONO_CASE(3) MONO_CASE(4) MONO_CASE(5)
    MONO_CASE(6) MONO_CASE(7) MONO_CASE(8) MONO_CASE(9) MONO_CASE(10)
#undef MONO_CASE
    default: return nullptr;
  }
}

}  // namespace btf
