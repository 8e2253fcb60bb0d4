// The gamma-grid family of the posterior-predictive kernels (btf_gg_predict.h): one compilation unit of its own.
// btf_analysis.hip launches them through the function pointers below.  gfx950 only.
#define BTF_GG_PRED_UNIT
#define BTF_PRED_UNIT           // (no extern declarations of the five families of btf_predict.hip: none is used here)
#include "btf_gg_predict.h"

namespace btf {

template __global__ void pred_kernel<PRED_FAM_GAMMA_GRID>(PredArgs);
template __global__ void pred_score_kernel<PRED_FAM_GAMMA_GRID>(PredArgs);

GgPredKernel gg_pred_fn() { return pred_kernel<PRED_FAM_GAMMA_GRID>; }
GgPredKernel gg_pred_score_fn() { return pred_score_kernel<PRED_FAM_GAMMA_GRID>; }
GgPredBatchKernel gg_pred_batch_fn() { return gg_pred_batch_kernel; }

}  // namespace btf
