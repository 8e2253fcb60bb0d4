// The dose-response likelihood (doseresponse/empirical_bayes.py:9-33, fit.py:28-38): an empirical-Bayes mixture of
// gammas over a grid of initial cell-population means, ESS / GASS likelihood family ESS_FAM_GAMMA_GRID (btf_ess.h).
// Component g = 1..G: shape a_g, scale s_g, weight p_g (used as given).  A cell with linear predictor eta = w.v and
// observed replicates y_r (S1 = sum_r y, L = sum_r log y, cnt of them) contributes
//     log sum_g p_g prod_r Gamma(y_r; a_g, scale = s_g eta)
//   = logsumexp_g [ log p_g + a_g (L - cnt log eta) - S1 / (s_g eta) - cnt (a_g log s_g + lgamma a_g) ] - L
// (the reference's nansum leaves a cell without observations at log sum_g p_g; eta <= 0 on an observed cell is -inf).
// The table is uploaded once (btf_set_likelihood_table) as {log p_g, a_g, 1 / s_g, a_g log s_g + lgamma a_g} per
// component with p_g > 0, and staged in LDS by every workgroup; L is a per-cell statistic in both layouts of S1
// (btf_set_data_logsum).  One pass over the components per (cell, candidate): one exp each (online logsumexp), one log
// and one division per (cell, candidate); exp / log from the LDS tables of btf_device.h.
//
//   gg_ll_rows_kernel<K> / gg_ll_cols_kernel<K>   the whole-state passes (poisson_ll_rows/cols_kernel of btf_ess.h)
//   gg_eval_kernel<ROWS, EP>                      the GASS candidates (gass_eval_kernel of btf_gass.h): lanes =
//                                                 candidates, the second 64 skipped when the chain has at most 64
//   gg_logsum_kernel                              L = sum_r log y of every cell, and a flag for an observed y <= 0
// Every sum has a fixed order (no float atomics): two calls give identical bits.
#pragma once
#if defined(BTF_GAMMA_GRID_UNIT) || defined(BTF_GG_CRIT_UNIT) || defined(BTF_SLICE_FOLD_UNIT) || defined(BTF_SLICE_FOLD_COLS_UNIT) || \
    defined(BTF_SLICE_FOLD_DEPTH_UNIT)
#include "btf_gass.h"
#else      // host code that needs the table's types alone (btf_ctx.h, btf_gg_criteria.h): no sampler kernels
#include "btf_device.h"
namespace btf { struct GassEvalArgs; }
#endif
#include <cmath>
#include <vector>

namespace btf {

constexpr int GG_MAXG = 128;

struct GgComp { double lp, a, b, c; };      // log p, shape, 1 / scale, shape log scale + lgamma(shape)

struct GgTab {
  const double* L;            // per-cell sum of log y, in the layout of the statistic the kernel reads
  const GgComp* tab; int G;   // components with p > 0
  double lsp;                 // log sum_g p_g: the value of a cell without observations
};

// the whole-state passes: the arguments of poisson_ll_rows_kernel / poisson_ll_cols_kernel, counts as bytes, f64 or
// the constant Rc (C8 == Cd == nullptr)
struct GgLLArgs {
  const double* A; const unsigned char* C8; const double* Cd; double Rc;
  const double* W; const double* V;
  int ncols, nl, ld, T;
  const int* done; int per_row;
  double* part;
};

// The table of the predictive draw (btf_gg_predict.h), laid out [a | s | c] with G entries each, every component of the
// table as given (a zero weight stays in its place and is never chosen): shape a_g, scale s_g and the cumulative weight
// c_g = sum_{h<=g} w_h, w_g = p_g / sum_h p_h.  Both sums are accumulated once, in ascending g, in fp64, here on the
// host, so that every call that holds the same table draws from the same bits.  From the last component with p_g > 0 on,
// c_g = 2: a uniform that round-off left at or above the last cumulative weight takes that component.
// mbar = sum_g w_g a_g s_g in ascending g: E[y | eta] = eta mbar.  false: a table btf_set_likelihood_table refuses.
inline bool gg_pred_table(const double* shape, const double* scale, const double* prob, int G, std::vector<double>& tab, double& mbar) {
  if (!shape || !scale || !prob || G < 1 || G > GG_MAXG) return false;
  double psum = 0.0;
  int last = -1;
  for (int g = 0; g < G; ++g) {
    const double a = shape[g], s = scale[g], p = prob[g];
    if (!std::isfinite(a) || !std::isfinite(s) || !std::isfinite(p) || !(a > 0.0) || !(s > 0.0) || !(p >= 0.0)) return false;
    psum += p;
    if (p > 0.0) last = g;
  }
  if (last < 0) return false;
  tab.assign((size_t)3 * G, 0.0);
  double c = 0.0;
  mbar = 0.0;
  for (int g = 0; g < G; ++g) {
    const double w = prob[g] / psum;
    c += w;
    mbar += w * shape[g] * scale[g];
    tab[g] = shape[g];
    tab[(size_t)G + g] = scale[g];
    tab[(size_t)2 * G + g] = g < last ? c : 2.0;
  }
  return true;
}

// The table of the likelihood kernels: {log p_g, a_g, 1 / s_g, a_g log s_g + lgamma a_g} for every component with p_g > 0,
// in the order given, and lsp = log sum_g p_g.  0: built; 1: an entry that is not finite shape > 0, scale > 0, weight >= 0
// (or G outside 1..128); 2: every weight is zero.
inline int gg_comp_table(const double* shape, const double* scale, const double* prob, int G, std::vector<GgComp>& tab, double& lsp) {
  if (!shape || !scale || !prob || G < 1 || G > GG_MAXG) return 1;
  tab.clear();
  double psum = 0.0;
  for (int g = 0; g < G; ++g) {
    const double a = shape[g], s = scale[g], p = prob[g];
    if (!std::isfinite(a) || !std::isfinite(s) || !std::isfinite(p) || !(a > 0.0) || !(s > 0.0) || !(p >= 0.0)) return 1;
    psum += p;
    if (p > 0.0) tab.push_back(GgComp{std::log(p), a, 1.0 / s, a * std::log(s) + std::lgamma(a)});    // (p = 0: no term)
  }
  lsp = std::log(psum);
  return tab.empty() ? 2 : 0;
}

using GgLLKernel = void (*)(GgLLArgs, GgTab);
using GgEvalKernel = void (*)(GassEvalArgs, GgTab);
using GgLogsumKernel = void (*)(const double*, int, int, int, int, int, double*, int*);
// btf_gamma_grid.hip: the kernels by nembeds (nullptr outside 1..10) and layout, for Prof::launch in btf_abi.hip
GgLLKernel gg_ll_rows_fn(int K);
GgLLKernel gg_ll_cols_fn(int K);
GgEvalKernel gg_eval_fn(bool rows, bool ep);
GgLogsumKernel gg_logsum_fn();

// the cell term, shared by this unit's kernels, the criteria kernels of btf_gg_criteria.h (BTF_GG_CRIT_UNIT) and the
// slice fold-in kernels of btf_slice_fold.h (BTF_SLICE_FOLD_UNIT), btf_slice_fold_cols.h (BTF_SLICE_FOLD_COLS_UNIT) and
// btf_slice_fold_depth.h (BTF_SLICE_FOLD_DEPTH_UNIT)
#if defined(BTF_GAMMA_GRID_UNIT) || defined(BTF_GG_CRIT_UNIT) || defined(BTF_SLICE_FOLD_UNIT) || defined(BTF_SLICE_FOLD_COLS_UNIT) || \
    defined(BTF_SLICE_FOLD_DEPTH_UNIT)
// table and exp / log tables into LDS (then a barrier, by the caller)
__device__ __forceinline__ void gg_stage(const GgTab& t, GgComp* tab, double2* ltab, double2* etab) {
  for (int g = threadIdx.x; g < t.G; g += blockDim.x) tab[g] = t.tab[g];
  log_table_build(ltab);
  exp_table_build(etab);
}

// the cell's log-likelihood at eta; X = S1 / eta, Y = L - cnt log eta
__device__ __forceinline__ double gg_term(double s1, double L, double cnt, double eta, const GgComp* __restrict__ tab, int G, double lsp,
                                          const double2* __restrict__ ltab, const double2* __restrict__ etab) {
  if (!(cnt > 0.0)) return lsp;
  if (!(eta > 0.0)) return -INFINITY;
  const double X = s1 / eta, Y = fma(-cnt, log_tab(eta, ltab), L);
  double m = -INFINITY, s = 0.0;
  for (int g = 0; g < G; ++g) {
    const GgComp q = tab[g];
    const double t = fma(-q.b, X, fma(q.a, Y, fma(-cnt, q.c, q.lp)));
    const double d = t - m;
    // exp(-|d|) (clamped: below e^-699 a term is lost against s >= 1 either way); the larger of t, m becomes the reference
    const double e = exp_tab(fmax(-fabs(d), -699.0), etab);
    s = d > 0.0 ? fma(s, e, 1.0) : s + e;
    m = fmax(m, t);
  }
  if (!(m > -INFINITY)) return -INFINITY;
  return m + log_tab(s, ltab) - L;
}
#endif  // BTF_GAMMA_GRID_UNIT || BTF_GG_CRIT_UNIT || BTF_SLICE_FOLD_UNIT || BTF_SLICE_FOLD_COLS_UNIT || BTF_SLICE_FOLD_DEPTH_UNIT

#ifdef BTF_GAMMA_GRID_UNIT
template <int K>
__global__ __launch_bounds__(ESS_THREADS) void gg_ll_rows_kernel(GgLLArgs a, GgTab t) {
  __shared__ double red[ESS_THREADS / WAVE];
  __shared__ GgComp tab[GG_MAXG];
  __shared__ double2 ltab[LOGTAB_N], etab[LOGTAB_N];
  const int i = blockIdx.y;
  if (a.per_row && a.done[i]) return;
  if (!a.per_row && a.done[0]) return;
  gg_stage(t, tab, ltab, etab);
  __syncthreads();
  double w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = a.W[(size_t)i * K + k];
  double s = 0.0;
  for (int l = blockIdx.x * ESS_THREADS + threadIdx.x; l < a.ncols; l += gridDim.x * ESS_THREADS) {
    const double* __restrict__ v = a.V + (size_t)l * K;
    double eta = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) eta = fma(w[k], v[k], eta);
    const size_t o = (size_t)i * a.ld + l;
    const double cnt = a.C8 ? (double)a.C8[o] : (a.Cd ? a.Cd[o] : a.Rc);
    s += gg_term(a.A[o], t.L[o], cnt, eta, tab, t.G, t.lsp, ltab, etab);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double u = 0.0;
    for (int q = 0; q < ESS_THREADS / WAVE; ++q) u += red[q];
    a.part[(size_t)i * gridDim.x + blockIdx.x] = u;
  }
}

template <int K>
__global__ __launch_bounds__(ESS_THREADS) void gg_ll_cols_kernel(GgLLArgs a, GgTab t) {
  __shared__ double red[ESS_THREADS / WAVE];
  __shared__ GgComp tab[GG_MAXG];
  __shared__ double2 ltab[LOGTAB_N], etab[LOGTAB_N];
  const int j = blockIdx.y, T = a.T;
  if (a.done[j]) return;
  gg_stage(t, tab, ltab, etab);
  __syncthreads();
  double s = 0.0;
  for (int i = blockIdx.x * ESS_THREADS + threadIdx.x; i < a.nl; i += gridDim.x * ESS_THREADS) {
    double w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = a.W[(size_t)i * K + k];
    for (int tt = 0; tt < T; ++tt) {
      const double* __restrict__ v = a.V + ((size_t)j * T + tt) * K;       // wave-uniform: scalar loads
      double eta = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) eta = fma(w[k], v[k], eta);
      const size_t o = ((size_t)j * T + tt) * a.ld + i;
      const double cnt = a.C8 ? (double)a.C8[o] : (a.Cd ? a.Cd[o] : a.Rc);
      s += gg_term(a.A[o], t.L[o], cnt, eta, tab, t.G, t.lsp, ltab, etab);
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double u = 0.0;
    for (int q = 0; q < ESS_THREADS / WAVE; ++q) u += red[q];
    a.part[(size_t)j * gridDim.x + blockIdx.x] = u;
  }
}

// gass_eval_kernel with the gamma-grid likelihood: the same cell tiles, the same order of every sum (so the same
// partial-sum layout, nsplit and EP quadratic form), L staged beside S1 and cnt.  A cell is wave-uniform, so the
// component loop and the table reads are too; only eta differs between the lanes.
template <bool ROWS, bool EP>
__global__ __launch_bounds__(GASS_THREADS) void gg_eval_kernel(GassEvalArgs a, GgTab t) {
  __shared__ double e0s[GASS_CT], e1s[GASS_CT], s1s[GASS_CT], cns[GASS_CT], lgs[GASS_CT];
  __shared__ double ems[EP ? GASS_CT : 1];
  __shared__ double q6s[EP ? GASS_THREADS / WAVE : 1][6];
  double q6[EP ? 6 : 1] = {};
  __shared__ double red[GASS_THREADS / WAVE][GASS_MAXC];
  __shared__ GgComp tab[GG_MAXG];
  __shared__ double2 ltab[LOGTAB_N], etab[LOGTAB_N];
  gg_stage(t, tab, ltab, etab);                 // (the tile loop's first barrier publishes it)
  const int ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = a.K, T = a.T;
  const int nth = a.ntheta[ch];
  const bool two = nth > 64;                    // wave-uniform: chains with at most 64 candidates skip the second half
  const double th0 = lane < nth ? a.thetas[(size_t)ch * GASS_MAXC + lane] : 0.0;
  const double th1 = lane + 64 < nth ? a.thetas[(size_t)ch * GASS_MAXC + lane + 64] : 0.0;
  double c0, s0, c1, s1;
  sincos(th0, &s0, &c0);
  sincos(th1, &s1, &c1);
  double acc0 = 0.0, acc1 = 0.0;
  const int ncell = ROWS ? a.M * T : a.N * T;
  for (int base = (int)blockIdx.y * GASS_CT; base < ncell && nth > 0; base += GASS_CT * a.nsplit) {
    __syncthreads();
    for (int e = tid; e < GASS_CT; e += GASS_THREADS) {
      const int cell = base + e;
      double d0 = 0.0, d1 = 0.0, sv = 0.0, cv = 0.0, lv = 0.0, dm = 0.0;
      double2 mp = make_double2(0.0, 0.0);
      if (cell < ncell) {
        size_t o;
        const double* __restrict__ f;
        const double* __restrict__ x;
        const double* __restrict__ nu;
        const double* __restrict__ mu = nullptr;
        if constexpr (ROWS) {          // chain = row i; cell = (j,t); statistics A_v[i][cell]
          f = a.F + (size_t)cell * K;
          x = a.X0 + (size_t)ch * K; nu = a.Nu + (size_t)ch * K;
          if constexpr (EP) mu = a.Mu + (size_t)ch * K;
          o = (size_t)ch * a.ld + cell;
        } else {                       // chain = column j; cell = (t, i) with i fastest; statistics A_wT[(j,t)][i]
          const int tt = cell / a.N, i = cell - tt * a.N;
          f = a.F + (size_t)i * K;
          x = a.X0 + ((size_t)ch * T + tt) * K; nu = a.Nu + ((size_t)ch * T + tt) * K;
          if constexpr (EP) mu = a.Mu + ((size_t)ch * T + tt) * K;
          o = ((size_t)ch * T + tt) * a.ld + i;
        }
        for (int k = 0; k < K; ++k) { d0 = fma(x[k], f[k], d0); d1 = fma(nu[k], f[k], d1); }
        sv = a.A[o];
        cv = a.C8 ? (double)a.C8[o] : (a.Cd ? a.Cd[o] : a.Rc);
        lv = t.L[o];
        if constexpr (EP) {
          for (int k = 0; k < K; ++k) dm = fma(mu[k], f[k], dm);
          mp = a.ep[(size_t)ch * ncell + cell];
        }
      }
      e0s[e] = d0; e1s[e] = d1; s1s[e] = sv; cns[e] = cv; lgs[e] = lv;
      if constexpr (EP) {
        ems[e] = dm;
        const double hp = 0.5 * mp.y, r = dm - mp.x;
        q6[0] = fma(hp * d0, d0, q6[0]); q6[1] = fma(hp * d1, d1, q6[1]); q6[2] = fma(hp * d0, d1, q6[2]);
        q6[3] = fma(hp * d0, r, q6[3]); q6[4] = fma(hp * d1, r, q6[4]); q6[5] = fma(hp * r, r, q6[5]);
      }
    }
    __syncthreads();
    const int lim = min(GASS_CT, ncell - base);
    for (int e = wave; e < lim; e += GASS_THREADS / WAVE) {
      const double d0 = e0s[e], d1 = e1s[e], sv = s1s[e], cv = cns[e], lv = lgs[e];
      const double dm = EP ? ems[e] : 0.0;
      acc0 += gg_term(sv, lv, cv, fma(c0, d0, s0 * d1) + dm, tab, t.G, t.lsp, ltab, etab);
      if (two) acc1 += gg_term(sv, lv, cv, fma(c1, d0, s1 * d1) + dm, tab, t.G, t.lsp, ltab, etab);
    }
  }
  red[wave][lane] = acc0;
  red[wave][lane + 64] = acc1;
  if constexpr (EP) {
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      double v = q6[q];
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
      if (lane == 0) q6s[wave][q] = v;
    }
  }
  __syncthreads();
  if (tid < GASS_MAXC) {
    double s = 0.0;
    for (int w = 0; w < GASS_THREADS / WAVE; ++w) s += red[w][tid];
    if constexpr (EP) {
      double Q[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) { double v = 0.0; for (int w = 0; w < GASS_THREADS / WAVE; ++w) v += q6s[w][q]; Q[q] = v; }
      double sn = 0.0, cs = 1.0;
      if (tid < nth) sincos(a.thetas[(size_t)ch * GASS_MAXC + tid], &sn, &cs);
      s += cs * cs * Q[0] + sn * sn * Q[1] + 2.0 * (cs * sn * Q[2] + cs * Q[3] + sn * Q[4]) + Q[5];
      if (blockIdx.y == 0) s += a.epc[ch];
    }
    if (a.nsplit == 1) a.ll[(size_t)ch * GASS_MAXC + tid] = tid < nth ? s : -INFINITY;
    else a.ll[((size_t)ch * a.nsplit + blockIdx.y) * GASS_MAXC + tid] = s;
  }
}

// Y slab [rows][cols][R] -> L[(transposed ? col*ld + row : row*ld + col)] = sum of log y over the observed replicates
// (the layouts of stats_kernel); *bad = 1 if an observed y is not positive
static __global__ __launch_bounds__(256) void gg_logsum_kernel(const double* __restrict__ Y, int rows, int cols, int R, int ld,
                                                              int transposed, double* __restrict__ L, int* __restrict__ bad) {
  const size_t cells = (size_t)rows * cols;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < cells; idx += (size_t)gridDim.x * blockDim.x) {
    size_t row, col;
    if (transposed) { col = idx / rows; row = idx - col * rows; }
    else { row = idx / cols; col = idx - row * cols; }
    const size_t cell = row * cols + col;
    double s = 0.0;
    bool neg = false;
    for (int r = 0; r < R; ++r) {
      const double y = Y[cell * R + r];
      if (y == y) { if (y > 0.0) s += log(y); else neg = true; }
    }
    L[transposed ? col * ld + row : row * ld + col] = s;
    if (neg) *bad = 1;
  }
}
#endif  // BTF_GAMMA_GRID_UNIT

}  // namespace btf
