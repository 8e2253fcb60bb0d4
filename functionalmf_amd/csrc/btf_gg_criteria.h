// Model-selection criteria for the gamma-grid likelihood: the per-curve log-likelihood over the kept samples
// (BTF_K_CRITERIA), family CRIT_FAM_GAMMA_GRID of btf_crit_eval / btf_crit_loo.
//
// Reference: the hand-made DIC of doseresponse/select_btf.py:9-23 under the likelihood of doseresponse/empirical_bayes.py.
// The cell term is a log-sum-exp over the G <= 128 components of a function of three per-cell statistics (S1 = sum_r y,
// L = sum_r log y, cnt), so it is no crit_term<FAM> plus a per-curve constant: it is gg_term of btf_gamma_grid.h itself,
// and the kernel below is crit_kernel (btf_criteria.h) around it - the same geometry, the same outputs, the same order of
// every sum, so that crit_total_kernel, the PSIS kernels of btf_loo.h and criteria.combine take its results unchanged.
//
//   gg_crit_kernel<K>       one workgroup per (column j, 64 rows), one lane per row, GGC_WAVES waves over depth chunks of
//                           GGC_TC cells, samples in blocks of GGC_SB: per curve the online log-sum-exp and Welford
//                           accumulators in ascending sample order, tot_part[s][wg], pw[S][N][M], mu[M][T][N] = sum_s w.v
//   gg_crit_plugin_kernel   ll of every curve at Mu-bar = mu / S, into curve[4]
//
// Cell values are gg_term's: a cell without observations inside an observed curve contributes log sum_g p_g, an observed
// cell with w.v <= 0 gives -inf.  A curve without any observation counts exactly 0 (as for every other family).
//
// Resources.  LDS: the component table (4 KiB), the log / exp tables (2 KiB each) and part[GGC_WAVES][GGC_SB][64] doubles,
// all static.  With crit_kernel's block of 32 samples that would be 72 KiB, over the static limit; this kernel is bound by
// the G exponentials per (cell, sample), not by re-reading 24 B of statistics per cell per sample block, so it takes
// GGC_SB = 16: 40 KiB, and two (three) workgroups fit a CU's 160 KiB.  Registers: a chunk holds 16 cells x (S1, L, cnt, mu).
// One pass over the components per (cell, sample); every lane reads the same component, so the table reads are wave-uniform
// (LDS broadcasts).  No floating-point atomics: every sum has a fixed order, two calls agree bit for bit.
#pragma once
#include "btf_criteria.h"
#include "btf_gamma_grid.h"

namespace btf {

constexpr int CRIT_FAM_GAMMA_GRID = ESS_FAM_GAMMA_GRID;
static_assert(CRIT_FAM_GAMMA_GRID == 5 && CRIT_FAM_GAMMA_GRID == CRIT_FAM_COUNT, "family 5 follows the five of crit_kernel");
constexpr int GGC_WAVES = CRIT_WAVES;   // waves per workgroup
constexpr int GGC_TC = CRIT_TC;         // depth cells per chunk (statistics and plug-in sums held in registers)
constexpr int GGC_SB = 16;              // samples per block: part[4][16][64] doubles = 32 KiB beside 8 KiB of tables

// CritArgs (c0 / c1 / noise / par unused) and the table; GgTab::L is the slot's [M][T][N] log-sum statistic
using GgCritKernel = void (*)(CritArgs, GgTab);
// btf_gg_criteria.hip: the kernel by nembeds (nullptr outside 1..10), for launch_counted in btf_analysis.hip
GgCritKernel gg_crit_fn(int K);
GgCritKernel gg_crit_plugin_fn();

#ifdef BTF_GG_CRIT_UNIT
// does curve (lane's row, j) hold an observation?  (all lanes of the wave: T coalesced loads)
__device__ __forceinline__ bool gg_crit_observed(const double* __restrict__ cnt, int j, int T, int N, int ic) {
  bool any = false;
  for (int t = 0; t < T; ++t) any |= cnt[((size_t)j * T + t) * N + ic] > 0.0;
  return any;
}

template <int K>
__global__ __launch_bounds__(GGC_WAVES * WAVE) void gg_crit_kernel(CritArgs a, GgTab g) {
  __shared__ double part[GGC_WAVES][GGC_SB][WAVE];
  __shared__ GgComp tab[GG_MAXG];
  __shared__ double2 ltab[LOGTAB_N], etab[LOGTAB_N];
  gg_stage(g, tab, ltab, etab);
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int j = blockIdx.y;
  const int i = blockIdx.x * WAVE + lane;
  const bool row_ok = i < a.N;
  const int ic = row_ok ? i : a.N - 1;                 // clamped row for the loads of the lanes past the end
  const int N = a.N, M = a.M, T = a.T;
  const int nch = (T + GGC_TC - 1) / GGC_TC;
  const int nwg = gridDim.x * gridDim.y, wg = blockIdx.y * gridDim.x + blockIdx.x;
  bool live = false;                                   // wave 0: a row of the tensor and a curve with an observation
  if (wv == 0) live = row_ok && gg_crit_observed(a.cnt, j, T, N, ic);
  double mx = -INFINITY, se = 0.0, mean = 0.0, m2 = 0.0;      // wave 0: the curve's running statistics
  for (int sb0 = 0; sb0 < a.S; sb0 += GGC_SB) {
    const int nb = min(GGC_SB, a.S - sb0);
    for (int ch = wv; ch < nch; ch += GGC_WAVES) {
      const int t0 = ch * GGC_TC, tn = min(GGC_TC, T - t0);
      double s1[GGC_TC], lg[GGC_TC], cn[GGC_TC], mu[GGC_TC];
#pragma unroll
      for (int u = 0; u < GGC_TC; ++u) {
        const size_t o = ((size_t)j * T + t0 + (u < tn ? u : 0)) * N + ic;
        s1[u] = u < tn ? a.S1[o] : 0.0;
        lg[u] = u < tn ? g.L[o] : 0.0;
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
        for (int u = 0; u < GGC_TC; ++u) {
          if (u < tn) {
            double eta = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) eta = fma(w[k], vp[u * K + k], eta);
            mu[u] += eta;
            acc += gg_term(s1[u], lg[u], cn[u], eta, tab, g.G, g.lsp, ltab, etab);
          }
        }
        if (ch == wv) part[wv][sl][lane] = acc;
        else part[wv][sl][lane] += acc;
      }
      if (row_ok) {
#pragma unroll
        for (int u = 0; u < GGC_TC; ++u)
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
        for (int w = 0; w < GGC_WAVES; ++w) sum += part[w][sl][lane];
        const double ll = live ? sum : 0.0;
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

// ll of every curve at the plug-in Mu-bar = mu / S, into curve[4][N][M].  One lane per row, one workgroup per
// (column, 64 rows).
static __global__ __launch_bounds__(WAVE) void gg_crit_plugin_kernel(CritArgs a, GgTab g) {
  __shared__ GgComp tab[GG_MAXG];
  __shared__ double2 ltab[LOGTAB_N], etab[LOGTAB_N];
  gg_stage(g, tab, ltab, etab);
  __syncthreads();
  const int i = blockIdx.x * WAVE + threadIdx.x, j = blockIdx.y;
  if (i >= a.N) return;
  const double inv = 1.0 / a.S;
  double acc = 0.0;
  bool any = false;
  for (int t = 0; t < a.T; ++t) {
    const size_t o = ((size_t)j * a.T + t) * a.N + i;
    const double cn = a.cnt[o];
    any |= cn > 0.0;
    acc += gg_term(a.S1[o], g.L[o], cn, a.mu[o] * inv, tab, g.G, g.lsp, ltab, etab);
  }
  a.curve[4 * (size_t)a.N * a.M + (size_t)i * a.M + j] = any ? acc : 0.0;
}
#endif  // BTF_GG_CRIT_UNIT

}  // namespace btf
