// Posterior predictive of the gamma-grid likelihood  (btf_predict_gg_eval, btf_predict_gg_batch)
//
// Reference: doseresponse/fit.py:475-478 (likelihood.sample(Mu_hat[None,i,j], size=[100, S, ndepth]) and the 5 / 95
// percentiles per curve, in a Python loop over every (cell line, drug)), empirical_bayes.py:21-27 (sample).  The sixth
// family of btf_predict.h: its draw / sort / reduce kernels are instantiated here with the draw below, nothing of them
// is restated.
//
// The draw.  y | eta = eta s_g Gamma(a_g, 1), the component g chosen with the weights w_g = p_g / sum_h p_h of the
// fitted likelihood.  (The reference's sample picks g by np.random.choice(G): uniformly, whatever mean_probs says.  A
// table with equal weights gives that.)  Draw number d of a cell is a pure function of (seed, table, eta, global draw
// index): PredRng(seed, family 5, index); its first uniform u picks the smallest g with u < c_g, c the cumulative
// weights of gg_pred_table (btf_gamma_grid.h: summed once on the host; a zero weight is never chosen; from the last
// positive weight on c = 2, so round-off cannot leave u without a component); pred_gamma(a_g) goes on with the same
// generator; y = (eta s_g) x.  eta <= 0 or nan gives nan.  Components are drawn per replicated observation - the
// marginal predictive of one new observation - where the likelihood shares one among the replicates of a cell.
// E[y | eta] = eta mbar, mbar = sum_g w_g a_g s_g: the kernels carry mbar as the family's parameter (PredArgs::par).
//
// The table ([a | s | c], 3 G doubles, 3 KiB at G = 128) is staged into static LDS once per workgroup, beside the dynamic
// [cells][P] rows.  The search over c is a fixed seven-step bisection in LDS; it is over before the gamma loop starts:
// one candidate per trip and lane, no loop nested in another (the rule of btf_predict.h).  No floating-point atomics.
//
// The sampler is __host__ __device__, as those of btf_predict.h.
#pragma once
#include "btf_gamma_grid.h"     // GG_MAXG, gg_pred_table
#include "btf_predict.h"

namespace btf {

constexpr int GGP_TAB_DOUBLES = 3 * GG_MAXG;      // static LDS of a workgroup, beside its rows

// the smallest g with u < c[g]; c ascending, c[G - 1] > u (gg_pred_table), 1 <= G <= GG_MAXG
__host__ __device__ inline int pred_gg_component(double u, const double* c, int G) {
  int g = 0;                                      // = the number of c's <= u
#pragma unroll
  for (int step = GG_MAXG / 2; step > 0; step >>= 1)
    if (g + step <= G && c[g + step - 1] <= u) g += step;
  return g;
}

// y | eta from the table tab = [a | s | c]; *comp: the component (-1 where eta gives no draw)
__host__ __device__ inline double pred_gg_draw(double eta, const double* tab, int G, PredRng& rng, int* comp) {
  *comp = -1;
  if (!(eta > 0.0)) return NAN;
  double u, spare;
  rng.uniform2(u, spare);
  const int g = pred_gg_component(u, tab + 2 * G, G);
  *comp = g;
  return eta * tab[G + g] * pred_gamma(tab[g], rng);
}

template <>
__host__ __device__ inline double pred_mean<PRED_FAM_GAMMA_GRID>(double eta, double mbar) { return eta > 0.0 ? eta * mbar : NAN; }

using GgPredKernel = void (*)(PredArgs);
using GgPredBatchKernel = void (*)(const double*, const double*, int, long long, unsigned long long, double*, int*);
// btf_gg_predict.hip: the family's kernels, for the launches of btf_analysis.hip
GgPredKernel gg_pred_fn();
GgPredKernel gg_pred_score_fn();
GgPredBatchKernel gg_pred_batch_fn();

#if defined(BTF_GG_PRED_UNIT) && defined(__HIPCC__)
// the table into LDS, by every thread of the workgroup (3 G <= GGP_TAB_DOUBLES: the entry points' check)
__device__ __forceinline__ const double* gg_pred_stage(const double* __restrict__ gg, int G) {
  __shared__ double tab[GGP_TAB_DOUBLES];
  for (int k = threadIdx.x; k < 3 * G; k += blockDim.x) tab[k] = gg[k];
  __syncthreads();
  return tab;
}

template <>
__device__ __forceinline__ const double* pred_stage<PRED_FAM_GAMMA_GRID>(const PredArgs& a) { return gg_pred_stage(a.gg, a.gg_G); }

template <>
__device__ __forceinline__ double pred_aux<PRED_FAM_GAMMA_GRID>(const PredArgs& a, int, int, int, int) { return a.par; }

template <>
__device__ inline double pred_draw<PRED_FAM_GAMMA_GRID>(double eta, double, unsigned long long seed, unsigned long long g,
                                                        const double* tab, int G) {
  PredRng rng(seed, PRED_FAM_GAMMA_GRID, g);
  int comp;
  return pred_gg_draw(eta, tab, G, rng, &comp);
}

// out[i]: draw number i at eta[i]; comp[i] (may be null): its component
__global__ __launch_bounds__(PRED_THREADS) void gg_pred_batch_kernel(const double* __restrict__ eta, const double* __restrict__ gg, int G,
                                                                    long long n, unsigned long long seed, double* __restrict__ out,
                                                                    int* __restrict__ comp) {
  const double* tab = gg_pred_stage(gg, G);
  const long long i = (long long)blockIdx.x * PRED_THREADS + threadIdx.x;
  if (i >= n) return;
  PredRng rng(seed, PRED_FAM_GAMMA_GRID, (unsigned long long)i);
  int g;
  out[i] = pred_gg_draw(eta[i], tab, G, rng, &g);
  if (comp) comp[i] = g;
}
#endif  // BTF_GG_PRED_UNIT

}  // namespace btf
