// Model-selection criteria for the conjugate Negative-Binomial model: the per-curve log-likelihood over the kept samples
// with the SAMPLED rate R_s of every sample (BTF_K_CRITERIA; btf_nb_crit_eval / btf_nb_crit_loo).
//
// Reference: _BayesianModel.select_hyperparams_DIC (genlasso.py:69-136) on the Negative-Binomial logprob (factor.py:462-563).
//   ll_s(i,j) = sum over observed (t,r) of lgamma(y+R) - lgamma(R) - lgamma(y+1) + y eta - (y+R) softplus(eta),
//   eta = w_i^s . v_jt^s (not clipped), R = R_s(i,j,t): one rate tensor per kept sample, full or shared along each of rows,
//   columns and depth (the model's rdims).  Family 4 of crit_kernel has ONE known rate, so its lgamma(y+r) - lgamma(r) is a
//   constant of the data built on the host; here it is a function of (sample, observation), split off as a kernel of its own:
//
//   nb_crit_const_kernel<ROWS>   C[s][j][i] = sum over observed (t,r) of lgamma(y+R_s) - lgamma(R_s), s = 0..S (rate S is the
//                                plug-in's R-bar), from the slot's raw counts Yt [M][T*nreps][N] (NaN = missing).
//                                crit_kernel's geometry: one lane per row, a column per blockIdx.y, wave w takes the chunks
//                                w, w + CRIT_WAVES, ... of CRIT_TC consecutive (t,r) observations, held in registers over a
//                                block of CRIT_SB samples - the counts are read ceil((S+1) / CRIT_SB) times, not S + 1 times.
//                                Every observation goes through nb_lgamma_rise (btf_lgamma.h: product form for integer
//                                y <= 32, Stirling above).  Used where the rate varies along rows or depth.
//   nb_crit_const_tab_kernel     the same C where the rate is one number per (sample, column) - uniform over the workgroup's
//                                cells: per block of NBC_TSB = 4 samples a table lgamma(y + R_s) - lgamma(R_s), y < NB_TAB, in
//                                LDS (nb_rise_table: nb_build_table's scan for one rate), one LDS read per integer count
//                                below 1024; y >= 1024 and non-integer y through nb_lgamma_rise.  Measured at
//                                (512,256,64,4), S = 1000, scalar rate: 157 ms of kernels for the call against 809 ms with
//                                the direct kernel, so the table is kept there (DESIGN.md 4b''').
//   nb_crit_kernel<K, ROWS>      crit_kernel with family 4's term under the rate of (s,i,j,t), read through the layout
//                                strides (ROWS: per lane; otherwise wave-uniform), and C[s][j][i] added when the curve's
//                                sum is finished.  Outputs, order of every sum and the exact 0 of a curve without
//                                observations as crit_kernel: crit_total_kernel, the PSIS kernels (btf_loo.h) and
//                                criteria.combine take them unchanged.
//   nb_crit_plugin_kernel<ROWS>  ll at Mu-bar = mu / S and R-bar (rate S, C[S]) into curve[4].
//
// The sample-independent - sum lgamma(y+1) is the slot's c0, built on the host as for family 4.
// Order of the sums: inside a chunk t ascending then r ascending; the chunks of a wave ascending; the waves' parts in wave
// order.  No floating-point atomics: two calls agree bit for bit.
// Resources: static LDS part[CRIT_WAVES][CRIT_SB][64] doubles = 65536 B in the direct constant kernel and the main kernel
// (crit_kernel's figure, the static limit itself), 40992 B in the table form (tab[4][1024] + part[4][4][64] + 4 doubles),
// none in the plug-in kernel.  VGPRs: constant 98 / 102 (wave-uniform / per-lane rate), table form 143, main 196 - 213 /
// 228 - 245 for K = 1..10, plug-in 70 / 78; no VGPR spills, no scratch.  Device scratch of a call: 8 (S+1) N M bytes for C and
// 8 (S+1) extent bytes for the rates, beside crit_kernel's.
#pragma once
#include "btf_criteria.h"
#include "btf_lgamma.h"

namespace btf {

// the rates of a call: R[S + 1][ext]; the rate of (s,i,j,t) is R[s * ext + i * sr0 + j * sr1 + t * sr2] (a stride is 0
// along an axis the rate is shared across)
struct NbRate { const double* R; long long ext, sr0, sr1, sr2; };
struct NbConstArgs {
  const double* Y;            // [M][T * nreps][N] raw counts, NaN = missing
  int nreps, S1, N, M, T;     // S1 = S + 1 rate tensors
  NbRate r;
  double* C;                  // [S1][M][N]
};

using NbConstKernel = void (*)(NbConstArgs);
using NbCritKernel = void (*)(CritArgs, NbRate, const double*);
// btf_nb_criteria.hip: the kernels by nembeds (nullptr outside 1..10) and by whether the rate varies along rows
constexpr int NBC_TSB = 4;       // samples per block of the table form: tab[4][1024] + part[4][4][64] doubles = 40 KiB
NbConstKernel nb_crit_const_fn(bool rows);
NbConstKernel nb_crit_const_tab_fn();      // the rate shared along rows and depth (sr0 = sr2 = 0)
NbCritKernel nb_crit_fn(int K, bool rows);
NbCritKernel nb_crit_plugin_fn(bool rows);

#ifdef BTF_NB_CRIT_UNIT
template <bool ROWS>
__global__ __launch_bounds__(CRIT_WAVES * WAVE) void nb_crit_const_kernel(NbConstArgs a) {
  __shared__ double part[CRIT_WAVES][CRIT_SB][WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int j = blockIdx.y;
  const int i = blockIdx.x * WAVE + lane;
  const bool row_ok = i < a.N;
  const int ic = row_ok ? i : a.N - 1;                 // clamped row for the loads of the lanes past the end
  const int N = a.N, M = a.M;
  const int F = a.T * a.nreps;                         // (t,r) slots of a curve, t-major
  const int nch = (F + CRIT_TC - 1) / CRIT_TC;
  const long long rbase = (ROWS ? (long long)ic * a.r.sr0 : 0) + (long long)j * a.r.sr1;
  for (int sb0 = 0; sb0 < a.S1; sb0 += CRIT_SB) {
    const int nb = min(CRIT_SB, a.S1 - sb0);
    for (int ch = wv; ch < nch; ch += CRIT_WAVES) {
      const int f0 = ch * CRIT_TC, fn = min(CRIT_TC, F - f0);
      double y[CRIT_TC];
      long long to[CRIT_TC];                           // the rate's offset along depth (wave-uniform)
#pragma unroll
      for (int u = 0; u < CRIT_TC; ++u) {
        const size_t o = ((size_t)j * F + f0 + (u < fn ? u : 0)) * N + ic;
        y[u] = u < fn ? a.Y[o] : __builtin_nan("");
        to[u] = (long long)((f0 + (u < fn ? u : 0)) / a.nreps) * a.r.sr2;
      }
      for (int sl = 0; sl < nb; ++sl) {
        const double* __restrict__ rp = a.r.R + (size_t)(sb0 + sl) * a.r.ext + rbase;
        double r = rp[0];
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < CRIT_TC; ++u) {
          if (a.r.sr2) r = rp[to[u]];
          if (y[u] == y[u]) acc += nb_lgamma_rise(y[u], r);
        }
        if (ch == wv) part[wv][sl][lane] = acc;
        else part[wv][sl][lane] += acc;
      }
    }
    if (wv >= nch)
      for (int sl = 0; sl < nb; ++sl) part[wv][sl][lane] = 0.0;
    __syncthreads();
    if (wv == 0 && row_ok) {
      for (int sl = 0; sl < nb; ++sl) {
        double sum = 0.0;
#pragma unroll
        for (int w = 0; w < CRIT_WAVES; ++w) sum += part[w][sl][lane];
        a.C[((size_t)(sb0 + sl) * M + j) * N + i] = sum;
      }
    }
    __syncthreads();
  }
}

// tab[y] = sum_{k<y} log(r + k) = lgamma(y + r) - lgamma(r), y = 0..NB_TAB-1, by all 256 threads of the workgroup (4 entries
// each): the scan of nb_build_table (btf_kernels.h) for one rate
__device__ inline void nb_rise_table(double r, double* tab, double* wsum) {
  static_assert(NB_TAB == 4 * CRIT_WAVES * WAVE, "4 table entries per thread");
  const int k0 = 4 * threadIdx.x, lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  double l[4], run = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) { run += log(r + (k0 + q)); l[q] = run; }
  double incl = run;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const double up = __shfl_up(incl, d, WAVE);
    if (lane >= d) incl += up;
  }
  if (lane == WAVE - 1) wsum[wv] = incl;
  __syncthreads();
  double off = incl - run;                       // exclusive prefix inside the wave
  for (int u = 0; u < wv; ++u) off += wsum[u];
  if (threadIdx.x == 0) tab[0] = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) if (k0 + q + 1 < NB_TAB) tab[k0 + q + 1] = off + l[q];
  __syncthreads();
}

// The same C where the rate is one number per (sample, column) - shared along rows and depth, so uniform over the
// workgroup's cells: per block of NBC_TSB samples a table of lgamma(y + R_s) - lgamma(R_s) in LDS, one read per integer
// count below NB_TAB; every other count (y >= NB_TAB, non-integer y) through nb_lgamma_rise as above.
template <int TSB>
__global__ __launch_bounds__(CRIT_WAVES * WAVE) void nb_crit_const_tab_kernel(NbConstArgs a) {
  __shared__ double tab[TSB][NB_TAB];
  __shared__ double part[CRIT_WAVES][TSB][WAVE];
  __shared__ double wsum[CRIT_WAVES];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int j = blockIdx.y;
  const int i = blockIdx.x * WAVE + lane;
  const bool row_ok = i < a.N;
  const int ic = row_ok ? i : a.N - 1;
  const int N = a.N, M = a.M;
  const int F = a.T * a.nreps;
  const int nch = (F + CRIT_TC - 1) / CRIT_TC;
  const double* __restrict__ rj = a.r.R + (long long)j * a.r.sr1;
  for (int sb0 = 0; sb0 < a.S1; sb0 += TSB) {
    const int nb = min(TSB, a.S1 - sb0);
    for (int sl = 0; sl < nb; ++sl) nb_rise_table(rj[(size_t)(sb0 + sl) * a.r.ext], tab[sl], wsum);
    for (int ch = wv; ch < nch; ch += CRIT_WAVES) {
      const int f0 = ch * CRIT_TC, fn = min(CRIT_TC, F - f0);
      double y[CRIT_TC];
#pragma unroll
      for (int u = 0; u < CRIT_TC; ++u) {
        const size_t o = ((size_t)j * F + f0 + (u < fn ? u : 0)) * N + ic;
        y[u] = u < fn ? a.Y[o] : __builtin_nan("");
      }
      for (int sl = 0; sl < nb; ++sl) {
        const double r = rj[(size_t)(sb0 + sl) * a.r.ext];
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < CRIT_TC; ++u) {
          if (y[u] == y[u]) {
            const bool tabbed = y[u] < (double)NB_TAB && y[u] == floor(y[u]);      // (y >= 0: btf_crit_set_counts)
            const double tv = tab[sl][tabbed ? (int)y[u] : 0];
            acc += tabbed ? tv : nb_lgamma_rise(y[u], r);
          }
        }
        if (ch == wv) part[wv][sl][lane] = acc;
        else part[wv][sl][lane] += acc;
      }
    }
    if (wv >= nch)
      for (int sl = 0; sl < nb; ++sl) part[wv][sl][lane] = 0.0;
    __syncthreads();
    if (wv == 0 && row_ok) {
      for (int sl = 0; sl < nb; ++sl) {
        double sum = 0.0;
#pragma unroll
        for (int w = 0; w < CRIT_WAVES; ++w) sum += part[w][sl][lane];
        a.C[((size_t)(sb0 + sl) * M + j) * N + i] = sum;
      }
    }
    __syncthreads();
  }
}

template <int K, bool ROWS>
__global__ __launch_bounds__(CRIT_WAVES * WAVE) void nb_crit_kernel(CritArgs a, NbRate rt, const double* __restrict__ C) {
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
  const long long rbase = (ROWS ? (long long)ic * rt.sr0 : 0) + (long long)j * rt.sr1;
  double c0 = 0.0;
  if (wv == 0) c0 = a.c0[(size_t)ic * M + j];
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
        const double* __restrict__ rp = rt.R + (size_t)s * rt.ext + rbase + (long long)t0 * rt.sr2;
        double w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = wp[k];
        double r = rp[0];
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < CRIT_TC; ++u) {
          if (u < tn) {
            double eta = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) eta = fma(w[k], vp[u * K + k], eta);
            mu[u] += eta;
            if (rt.sr2) r = rp[u * rt.sr2];
            acc += crit_term<CRIT_FAM_NEGBIN>(s1[u], cn[u], eta, r);
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
        const double ll = row_ok ? (sum + C[((size_t)s * M + j) * N + ic]) + c0 : 0.0;
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

// ll of every curve at the plug-in Mu-bar = mu / S and R-bar (the rate tensor S, with its constant C[S]), into
// curve[4][N][M].  One lane per row, one workgroup per (column, 64 rows).
template <bool ROWS>
__global__ __launch_bounds__(WAVE) void nb_crit_plugin_kernel(CritArgs a, NbRate rt, const double* __restrict__ C) {
  const int i = blockIdx.x * WAVE + threadIdx.x, j = blockIdx.y;
  if (i >= a.N) return;
  const double inv = 1.0 / a.S;
  const double* __restrict__ rp = rt.R + (size_t)a.S * rt.ext + (ROWS ? (long long)i * rt.sr0 : 0) + (long long)j * rt.sr1;
  double acc = 0.0;
  for (int t = 0; t < a.T; ++t) {
    const size_t o = ((size_t)j * a.T + t) * a.N + i;
    acc += crit_term<CRIT_FAM_NEGBIN>(a.S1[o], a.cnt[o], a.mu[o] * inv, rp[(long long)t * rt.sr2]);
  }
  const size_t oc = (size_t)i * a.M + j;
  a.curve[4 * (size_t)a.N * a.M + oc] = (acc + C[((size_t)a.S * a.M + j) * a.N + i]) + a.c0[oc];
}
#endif  // BTF_NB_CRIT_UNIT

}  // namespace btf
