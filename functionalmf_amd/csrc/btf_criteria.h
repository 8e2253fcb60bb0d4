// Model-selection criteria: the per-curve log-likelihood over the kept samples  (BTF_K_CRITERIA)
//
// Reference: _BayesianModel.select_hyperparams_DIC (genlasso.py:69-136) on logprob (factor.py:262-264, :610-612,
// :1002-1005), and the hand-made DIC of doseresponse/select_btf.py:9-23.  What WAIC, DIC and held-out scoring are made
// of is ll_s(i,j): the normalised log-likelihood of curve (i,j) - every observed y_ijtr over depth and replicates - under
// kept sample s.  The (S,N,M,T) tensor of linear predictors w_i^s . v_jt^s is never formed: per curve this kernel keeps
// an online log-sum-exp (running max + rescaled sum) and a Welford mean / M2 over the samples in ascending order, per
// sample a per-workgroup partial of sum_ij ll_s, and per cell the sum over samples of w.v (the plug-in Mu-bar of the DIC).
//
// Statistics (btf_crit_set_data; functionalmf_amd/criteria.py builds them once per data tensor):
//   S1[j][t][i] = sum_r y,  cnt[j][t][i] = observed replicates (Binomial: trials)   - lanes along rows: loads coalesce
//   c0[i][j], c1[i][j]: the curve's normalising constant (family 3: Q = sum y^2 and n = observations)
// Families (the ESS link conventions of btf_ess.h, all with the state-independent terms added back):
//   0 Poisson, log link         sum_t S1 eta - cnt exp(eta)                                  + c0
//   1 Poisson, identity link    sum_t S1 log(eta) - cnt eta  (-inf where eta <= 0)           + c0
//   2 logit (Binomial / Bernoulli: S1 successes of cnt trials)  sum_t S1 eta - cnt softplus(eta)  + c0
//   3 Gaussian, variance v      (sum_t (S1 eta - cnt eta^2 / 2) - c0 / 2) / v - c1 log(2 pi v) / 2
//   4 Negative-Binomial, logit link, rate r   sum_t S1 eta - (S1 + cnt r) softplus(eta)      + c0
// Cells with cnt = 0 contribute exactly 0, so a curve without observations has ll = 0.
//
// Geometry: one workgroup per (column j, 64 rows), one lane per row, CRIT_WAVES waves.  The samples go in blocks of
// CRIT_SB; inside a block wave w takes the depth chunks w, w + CRIT_WAVES, ... of CRIT_TC cells: it loads the chunk's
// statistics into registers ONCE and runs over the block's samples (w_i^s: K per-lane loads; v_jt^s: wave-uniform,
// scalar loads), so the statistics are read once per block of samples, not once per sample.  Partial curve sums go to
// LDS [wave][sample][lane]; after a barrier wave 0 adds the waves' parts in a fixed order and folds the block into the
// per-curve accumulators.  No floating-point atomics: every sum has a fixed order, two calls agree bit for bit.
#pragma once
#include "btf_device.h"
#include <math.h>

namespace btf {

enum { CRIT_FAM_POISSON_LOG = 0, CRIT_FAM_POISSON_IDENTITY = 1, CRIT_FAM_LOGIT = 2, CRIT_FAM_GAUSSIAN = 3, CRIT_FAM_NEGBIN = 4,
       CRIT_FAM_COUNT = 5 };
constexpr int CRIT_WAVES = 4;     // waves per workgroup
constexpr int CRIT_TC = 16;       // depth cells per chunk (statistics and plug-in sums held in registers)
constexpr int CRIT_SB = 32;       // samples per block: the statistics are read ceil(S / CRIT_SB) times; LDS 64 KiB
constexpr int CRIT_OUT = 5;       // per-curve outputs: max-shifted sum of exp, max, mean, M2, ll at the plug-in

struct CritArgs {
  const double* S1; const double* cnt;   // [M][T][N]
  const double* c0; const double* c1;    // [N][M]
  const double* W;                       // [S][N][K]
  const double* V;                       // [S][M][T][K]
  const double* noise; long long noise_stride;   // family 3: per-sample variance noise[s * stride], or null: par
  double par;                            // family 3: the variance; 4: the rate r
  int S, N, M, T;
  double* mu;                            // [M][T][N]: sum over samples of w.v (the plug-in's Mu-bar times S)
  double* curve;                         // [CRIT_OUT][N][M]
  double* tot_part;                      // [S][workgroups]: per-workgroup partial of sum_ij ll_s
  double* pw;                            // [S][N][M] pointwise log-likelihoods, or null
};

__device__ __forceinline__ double crit_softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// one cell's state-dependent term (family 3: before the curve's 1 / v scaling)
template <int FAM>
__device__ __forceinline__ double crit_term(double s1, double cnt, double eta, double par) {
  if (!(cnt > 0.0)) return 0.0;
  if constexpr (FAM == CRIT_FAM_POISSON_LOG) return fma(s1, eta, -cnt * exp(eta));
  else if constexpr (FAM == CRIT_FAM_POISSON_IDENTITY) return eta > 0.0 ? fma(s1, log(eta), -cnt * eta) : -INFINITY;
  else if constexpr (FAM == CRIT_FAM_LOGIT) return fma(s1, eta, -cnt * crit_softplus(eta));
  else if constexpr (FAM == CRIT_FAM_GAUSSIAN) return eta * fma(-0.5 * cnt, eta, s1);
  else return fma(s1, eta, -fma(cnt, par, s1) * crit_softplus(eta));
}

// the curve's normalised log-likelihood from the sum of its terms
template <int FAM>
__device__ __forceinline__ double crit_finish(double a, double c0, double c1, double var) {
  if constexpr (FAM == CRIT_FAM_GAUSSIAN) return c1 > 0.0 ? fma(a - 0.5 * c0, 1.0 / var, -0.5 * c1 * log(6.283185307179586 * var)) : 0.0;
  else return a + c0;
}

template <int K, int FAM>
__global__ __launch_bounds__(CRIT_WAVES * WAVE) void crit_kernel(CritArgs a) {
  __shared__ double part[CRIT_WAVES][CRIT_SB][WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int j = blockIdx.y;
  const int i = blockIdx.x * WAVE + lane;
  const bool row_ok = i < a.N;
  const int ic = row_ok ? i : a.N - 1;                 // clamped row for the loads of the lanes past the end
  const int N = a.N, M = a.M, T = a.T;
  const int nch = (T + CRIT_TC - 1) / CRIT_TC;
  const int nwg = gridDim.x * gridDim.y, wg = blockIdx.y * gridDim.x + blockIdx.x;
  double c0 = 0.0, c1 = 0.0;
  if (wv == 0) { c0 = a.c0[(size_t)ic * M + j]; c1 = a.c1[(size_t)ic * M + j]; }
  double mx = -INFINITY, se = 0.0, mean = 0.0, m2 = 0.0;      // wave 0: the curve's running statistics
  for (int sb0 = 0; sb0 < a.S; sb0 += CRIT_SB) {
    const int nb = min(CRIT_SB, a.S - sb0);
    for (int ch = wv; ch < nch; ch += CRIT_WAVES) {
      const int t0 = ch * CRIT_TC, tn = min(CRIT_TC, T - t0);
      double s1[CRIT_TC], cn[CRIT_TC], mu[CRIT_TC];
#pragma unroll
      for (int u = 0; u < CRIT_TC; ++u) {
        const size_t o = ((size_t)j * T + t0 + (u < tn ? u : 0)) * N + ic;
        s1[u] = u < tn ? a.S1[o] : 0.0;
        cn[u] = u < tn ? a.cnt[o] : 0.0;
        mu[u] = 0.0;
      }
      for (int sl = 0; sl < nb; ++sl) {
        const int s = sb0 + sl;
        const double* __restrict__ wp = a.W + ((size_t)s * N + ic) * K;
        const double* __restrict__ vp = a.V + (((size_t)s * M + j) * T + t0) * K;
        double w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = wp[k];
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < CRIT_TC; ++u) {
          if (u < tn) {
            double eta = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) eta = fma(w[k], vp[u * K + k], eta);
            mu[u] += eta;
            acc += crit_term<FAM>(s1[u], cn[u], eta, a.par);
          }
        }
        if (ch == wv) part[wv][sl][lane] = acc;
        else part[wv][sl][lane] += acc;
      }
      if (row_ok) {
#pragma unroll
        for (int u = 0; u < CRIT_TC; ++u)
          if (u < tn) {
            const size_t o = ((size_t)j * T + t0 + u) * N + i;
            a.mu[o] = sb0 == 0 ? mu[u] : a.mu[o] + mu[u];
          }
      }
    }
    if (wv >= nch)
      for (int sl = 0; sl < nb; ++sl) part[wv][sl][lane] = 0.0;
    __syncthreads();
    if (wv == 0) {
      for (int sl = 0; sl < nb; ++sl) {
        const int s = sb0 + sl;
        double sum = 0.0;
#pragma unroll
        for (int w = 0; w < CRIT_WAVES; ++w) sum += part[w][sl][lane];
        const double var = (FAM == CRIT_FAM_GAUSSIAN && a.noise) ? a.noise[(size_t)s * a.noise_stride] : a.par;
        const double ll = row_ok ? crit_finish<FAM>(sum, c0, c1, var) : 0.0;
        // online log-sum-exp (-inf terms add nothing; all -inf leaves max -inf and sum 0: log-sum-exp -inf)
        if (ll > mx) { se = fma(se, exp(mx - ll), 1.0); mx = ll; }
        else if (ll != -INFINITY) se += exp(ll - mx);
        // Welford (a -inf sample makes the mean -inf and M2 nan, as np.var)
        const double d = ll - mean;
        mean += d / (double)(s + 1);
        m2 = fma(d, ll - mean, m2);
        if (a.pw && row_ok) a.pw[((size_t)s * N + i) * M + j] = ll;
        const double tot = wave_sum(ll);
        if (lane == 0) a.tot_part[(size_t)s * nwg + wg] = tot;
      }
    }
    __syncthreads();
  }
  if (wv == 0 && row_ok) {
    const size_t o = (size_t)i * M + j, NM = (size_t)N * M;
    a.curve[o] = se;
    a.curve[NM + o] = mx;
    a.curve[2 * NM + o] = mean;
    a.curve[3 * NM + o] = m2;
  }
}

// ll of every curve at the plug-in Mu-bar = mu / S and the mean variance (family 3: the mean of the per-sample noise,
// summed in sample order), into curve[4][N][M].  One lane per row, one workgroup per (column, 64 rows).
template <int FAM>
__global__ __launch_bounds__(WAVE) void crit_plugin_kernel(CritArgs a) {
  const int i = blockIdx.x * WAVE + threadIdx.x, j = blockIdx.y;
  double var = a.par;
  if (FAM == CRIT_FAM_GAUSSIAN && a.noise) {
    double sv = 0.0;
    for (int s = 0; s < a.S; ++s) sv += a.noise[(size_t)s * a.noise_stride];
    var = sv / a.S;
  }
  if (i >= a.N) return;
  const double inv = 1.0 / a.S;
  double acc = 0.0;
  for (int t = 0; t < a.T; ++t) {
    const size_t o = ((size_t)j * a.T + t) * a.N + i;
    acc += crit_term<FAM>(a.S1[o], a.cnt[o], a.mu[o] * inv, a.par);
  }
  const size_t oc = (size_t)i * a.M + j;
  a.curve[4 * (size_t)a.N * a.M + oc] = crit_finish<FAM>(acc, a.c0[oc], a.c1[oc], var);
}

// total_out[s] = sum over workgroups of tot_part[s][.], in workgroup order
static __global__ void crit_total_kernel(const double* __restrict__ tot_part, int S, int nwg, double* __restrict__ total) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  double t = 0.0;
  for (int w = 0; w < nwg; ++w) t += tot_part[(size_t)s * nwg + w];
  total[s] = t;
}

#define BTF_CRIT_SET(P, K)                                                                               \
  P void crit_kernel<K, 0>(CritArgs); P void crit_kernel<K, 1>(CritArgs); P void crit_kernel<K, 2>(CritArgs); \
  P void crit_kernel<K, 3>(CritArgs); P void crit_kernel<K, 4>(CritArgs);
#define BTF_CRIT_PLUGIN_SET(P)                                                                           \
  P void crit_plugin_kernel<0>(CritArgs); P void crit_plugin_kernel<1>(CritArgs); P void crit_plugin_kernel<2>(CritArgs); \
  P void crit_plugin_kernel<3>(CritArgs); P void crit_plugin_kernel<4>(CritArgs);

// instantiated in btf_criteria.hip (its own compilation unit), declared here for the C-ABI unit
#ifndef BTF_CRIT_UNIT
#define BTF_X extern template __global__
BTF_CRIT_SET(BTF_X, 1) BTF_CRIT_SET(BTF_X, 2) BTF_CRIT_SET(BTF_X, 3) BTF_CRIT_SET(BTF_X, 4) BTF_CRIT_SET(BTF_X, 5)
BTF_CRIT_SET(BTF_X, 6) BTF_CRIT_SET(BTF_X, 7) BTF_CRIT_SET(BTF_X, 8) BTF_CRIT_SET(BTF_X, 9) BTF_CRIT_SET(BTF_X, 10)
BTF_CRIT_PLUGIN_SET(BTF_X)
#undef BTF_X
#endif

}  // namespace btf
