// Posterior predictive checks: predictive p-values of whole-curve discrepancies  (btf_predict_check)
//
// The written definition is functionalmf_amd/checks.py (discrepancies, reference).  For every curve (i,j), kept sample s
// and rho < reps a replicated curve y_rep is drawn at the curve's observed slots (t, rep) - draw number
// g = cell n + s Rr + rho nreps + rep of pred_draw<FAM>, Rr = reps nreps, n = S Rr: the very draws btf_predict_eval makes
// with draws_per_sample = Rr - and five discrepancies T(y, theta_s) are formed for y_rep and for the data y:
//   chisq  sum (y - mu)^2 / v          max    max |y - mu| / sqrt(v)          total  sum y          zeros  #{y == 0}
//   lag1   sum_{t, t+1 defined} e_t e_{t+1} / sum_{t defined} e_t^2,   e_t = sum_rep (y - mu_t) / sqrt(v_t m_t)
// (sums over t ascending, then rep ascending, as plain adds; slots with v == 0 are left out of the first three).
//
// Geometry.  One workgroup per (row i, tile of CHK_TILE columns), CHK_THREADS lanes along the replicated sets
// e = s reps + rho, block after block of CHK_THREADS sets.  A lane keeps w_i^s in registers, walks the columns of the tile
// and their depths in order and holds the running discrepancies of y_rep and of y (and the lag-1 carry) in registers:
// every (curve, e) value is computed by one lane alone, so no result depends on the geometry.  The data of the curve (Y,
// trials) is read at wave-uniform addresses.  When a curve ends, the comparison bits become integer counts (ballot,
// popcount, an LDS integer add: exact in any order) and the sums for t_obs / t_rep meet in a fixed order: butterfly
// within the wave, the waves in wave order, the blocks of sets in block order.  The pooled discrepancies stay in the
// lane across the tile and are written once per (workgroup, e); chk_pool_kernel adds the workgroups in index order.
// A bad curve - one with a slot nothing can be drawn at (pred_drawable: eta <= 0 under the identity link, a missing trial
// count) - is found before the draws by the whole workgroup, draws nothing and is left out of the pool.
// No floating-point atomics.
#pragma once
#include "btf_predict.h"

namespace btf {

enum { CHK_CHISQ = 0, CHK_MAX = 1, CHK_LAG1 = 2, CHK_TOTAL = 3, CHK_ZEROS = 4, CHK_COUNT = 5 };
// what a lane accumulates per curve and pools per tile: lag1 as numerator, denominator and "has an adjacent pair"
enum { CHK_S_CHISQ = 0, CHK_S_MAX = 1, CHK_S_NUM = 2, CHK_S_DEN = 3, CHK_S_PAIR = 4, CHK_S_TOTAL = 5, CHK_S_ZEROS = 6, CHK_SLOTS = 7 };
enum { CHK_O_GE = 0, CHK_O_GT = 1, CHK_O_DEFINED = 2, CHK_O_SUM_OBS = 3, CHK_O_SUM_REP = 4, CHK_OUTS = 5 };   // per (curve, code)
constexpr int CHK_THREADS = 256;
constexpr int CHK_WAVES = CHK_THREADS / WAVE;
constexpr int CHK_MAX_K = 10;                  // nembeds at most (MAX_K of btf_ctx.h)
constexpr int CHK_TILE = 8;                     // columns per workgroup = the tile of the pooled sums (checks.POOL_TILE)
constexpr size_t CHK_PART_BYTES = (size_t)192 << 20;   // the pooled partials of one launch (the rows are chunked to fit)

// Var[y | eta, aux] beside pred_mean: aux = the variance (Gaussian), trials (logit), the rate r (Negative-Binomial)
template <int FAM>
__host__ __device__ inline double pred_var(double eta, double aux) {
  if constexpr (FAM == PRED_FAM_POISSON_LOG || FAM == PRED_FAM_POISSON_IDENTITY) return pred_mean<FAM>(eta, aux);
  else if constexpr (FAM == PRED_FAM_LOGIT) {
    const double e = exp(-fabs(eta));             // p (1 - p) = e / (1 + e)^2, either tail exact
    return aux * (e / ((1.0 + e) * (1.0 + e)));
  } else if constexpr (FAM == PRED_FAM_GAUSSIAN) return aux;
  else { const double e = exp(eta); return aux * e * (1.0 + e); }
}

// pred_draw<FAM>(eta, aux, ...) returns a number (its refusals, restated as a predicate; a Negative-Binomial draw whose
// gamma variate times exp(eta) overflows is still nan, and poisons what it enters)
template <int FAM>
__host__ __device__ inline bool pred_drawable(double eta, double aux) {
  if constexpr (FAM == PRED_FAM_GAUSSIAN) return aux >= 0.0 && eta == eta;
  else if constexpr (FAM == PRED_FAM_POISSON_LOG) { const double lam = exp(eta); return lam >= 0.0 && lam < INFINITY; }
  else if constexpr (FAM == PRED_FAM_POISSON_IDENTITY) return eta > 0.0 && eta < INFINITY;
  else if constexpr (FAM == PRED_FAM_LOGIT) return aux >= 0.0 && aux < INFINITY && aux == floor(aux) && eta == eta;
  else { const double lam = exp(eta); return aux > 0.0 && aux < INFINITY && lam >= 0.0 && lam < INFINITY; }
}

#ifdef __HIPCC__
struct ChkArgs {
  PredArgs p;                            // states, aux layout, trials, Y / nreps, S, N, M, T, K, seed (R = reps nreps)
  int reps, nsets;                       // replicated sets per sample, S reps
  int row0, rows, tiles;                 // this launch: rows row0 .. row0 + rows, tiles = ceil(M / CHK_TILE)
  const int* listed;                     // [N M] slot of a listed curve or -1, or null
  double* cur;                           // [CHK_OUTS][CHK_COUNT][N M]
  double* nobs;                          // [N M]
  double* part;                          // [rows tiles][2 (rep, obs)][CHK_SLOTS][nsets]
  double *t_obs, *t_rep;                 // listed curves: [L][CHK_COUNT][nsets] each (t_obs: the value of the set's sample)
};

// the running discrepancies of one curve under one state
struct ChkAcc {
  double v[CHK_SLOTS];
  double rsum, eprev;
  bool prevdef;
  __device__ __forceinline__ void curve_begin() {
#pragma unroll
    for (int k = 0; k < CHK_SLOTS; ++k) v[k] = 0.0;
    prevdef = false; eprev = 0.0;
  }
  __device__ __forceinline__ void depth_begin() { rsum = 0.0; }
  __device__ __forceinline__ void slot(double y, double mu, double var) {
    const double r = y - mu;
    if (var != 0.0) {
      v[CHK_S_CHISQ] += r * r / var;
      v[CHK_S_MAX] = fmax(v[CHK_S_MAX], fabs(r) / sqrt(var));
      rsum += r;
    }
    v[CHK_S_TOTAL] += y;
    v[CHK_S_ZEROS] += (y == 0.0) ? 1.0 : 0.0;
  }
  // the depth had m > 0 observed replicates
  __device__ __forceinline__ void depth_end(double var, double m) {
    if (var != 0.0) {
      const double e = rsum / sqrt(var * m);
      v[CHK_S_DEN] += e * e;
      if (prevdef) { v[CHK_S_NUM] += eprev * e; v[CHK_S_PAIR] = 1.0; }
      eprev = e; prevdef = true;
    } else prevdef = false;
  }
  __device__ __forceinline__ void depth_gap() { prevdef = false; }
  __device__ __forceinline__ double lag1() const {
    return (v[CHK_S_PAIR] != 0.0 && v[CHK_S_DEN] != 0.0) ? v[CHK_S_NUM] / v[CHK_S_DEN] : NAN;
  }
  __device__ __forceinline__ double value(int code) const {
    return code == CHK_CHISQ ? v[CHK_S_CHISQ] : code == CHK_MAX ? v[CHK_S_MAX] : code == CHK_LAG1 ? lag1()
         : code == CHK_TOTAL ? v[CHK_S_TOTAL] : v[CHK_S_ZEROS];
  }
};

__device__ __forceinline__ void chk_pool_add(double (&pool)[CHK_SLOTS], const ChkAcc& a) {
#pragma unroll
  for (int k = 0; k < CHK_SLOTS; ++k) pool[k] = (k == CHK_S_MAX) ? fmax(pool[k], a.v[k]) : pool[k] + a.v[k];
}

template <int FAM>
__global__ __launch_bounds__(CHK_THREADS) void chk_kernel(ChkArgs c) {
  __shared__ int s_cnt[CHK_TILE][3][CHK_COUNT];                 // ge, gt, defined
  __shared__ double s_sum[CHK_TILE][2][CHK_COUNT];              // t_obs, t_rep sums
  __shared__ double s_red[CHK_TILE][CHK_WAVES][2][CHK_COUNT];   // one block of sets: per wave
  __shared__ int s_nobs[CHK_TILE], s_bad[CHK_TILE];
  const PredArgs& a = c.p;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  const int rl = blockIdx.x % c.rows, tile = blockIdx.x / c.rows;        // row fastest: workgroups in flight share V
  const int i = c.row0 + rl, j0 = tile * CHK_TILE, nc = min(CHK_TILE, a.M - j0);
  const int T = a.T, nreps = a.nreps, K = a.K;
  const unsigned long long n = (unsigned long long)c.nsets * (unsigned long long)nreps;
  for (int e = tid; e < CHK_TILE * 3 * CHK_COUNT; e += CHK_THREADS) (&s_cnt[0][0][0])[e] = 0;
  for (int e = tid; e < CHK_TILE * 2 * CHK_COUNT; e += CHK_THREADS) (&s_sum[0][0][0])[e] = 0.0;
  if (tid < CHK_TILE) { s_nobs[tid] = 0; s_bad[tid] = 0; }
  __syncthreads();
  // ---- which curves of the tile are observed, which are bad: threads stride over (depth, sample)
  for (int cj = 0; cj < nc; ++cj) {
    const int j = j0 + cj;
    const size_t cell0 = ((size_t)i * a.M + j) * T;
    int no = 0;
    bool bad = false;
    for (int t = 0; t < T; ++t) {
      int m = 0;
      for (int r = 0; r < nreps; ++r) { const double y = a.Y[(cell0 + t) * nreps + r]; m += (y == y) ? 1 : 0; }
      no += m;
      if (m == 0) continue;                          // wave-uniform
      for (int s = tid; s < a.S; s += CHK_THREADS)
        bad |= !pred_drawable<FAM>(pred_eta(a, s, i, j * T + t), pred_aux<FAM>(a, s, i, j, t));
    }
    if (tid == 0) s_nobs[cj] = no;
    if (__ballot(bad) != 0ULL && lane == 0) atomicOr(&s_bad[cj], 1);
  }
  __syncthreads();
  // ---- the replicated sets, CHK_THREADS at a time
  const int nblocks = (c.nsets + CHK_THREADS - 1) / CHK_THREADS;
  for (int eb = 0; eb < nblocks; ++eb) {
    const int e = eb * CHK_THREADS + tid;
    const bool active = e < c.nsets;
    const int s = active ? e / c.reps : 0, rho = active ? e % c.reps : 0;
    double w[CHK_MAX_K];
    {
      const double* __restrict__ wp = a.W + ((size_t)s * a.N + i) * K;
#pragma unroll
      for (int k = 0; k < CHK_MAX_K; ++k) w[k] = k < K ? wp[k] : 0.0;
    }
    double pool_rep[CHK_SLOTS], pool_obs[CHK_SLOTS];
#pragma unroll
    for (int k = 0; k < CHK_SLOTS; ++k) { pool_rep[k] = 0.0; pool_obs[k] = 0.0; }
    for (int cj = 0; cj < nc; ++cj) {
      const int j = j0 + cj;
      const size_t curve = (size_t)i * a.M + j, cell0 = curve * T;
      const bool skip = s_nobs[cj] == 0 || s_bad[cj] != 0;         // workgroup-uniform
      const int slot = c.listed ? c.listed[curve] : -1;
      ChkAcc rep, obs;
      rep.curve_begin(); obs.curve_begin();
      if (!skip && active) {
        const double* __restrict__ vp = a.V + ((size_t)s * a.M + j) * T * K;
        for (int t = 0; t < T; ++t) {
          int m = 0;
          for (int r = 0; r < nreps; ++r) { const double y = a.Y[(cell0 + t) * nreps + r]; m += (y == y) ? 1 : 0; }
          if (m == 0) { rep.depth_gap(); obs.depth_gap(); continue; }
          double eta = 0.0;                           // pred_eta's chain of fused multiply-adds, w from registers
#pragma unroll
          for (int k = 0; k < CHK_MAX_K; ++k) if (k < K) eta = fma(w[k], vp[(size_t)t * K + k], eta);
          const double aux = pred_aux<FAM>(a, s, i, j, t);
          const double mu = pred_mean<FAM>(eta, aux), var = pred_var<FAM>(eta, aux);
          const unsigned long long g0 = (unsigned long long)(cell0 + t) * n + (unsigned long long)s * (unsigned long long)a.R +
                                        (unsigned long long)rho * (unsigned long long)nreps;
          rep.depth_begin(); obs.depth_begin();
          for (int r = 0; r < nreps; ++r) {
            const double y = a.Y[(cell0 + t) * nreps + r];
            if (y != y) continue;                     // wave-uniform
            rep.slot(pred_draw<FAM>(eta, aux, a.seed, g0 + (unsigned long long)r), mu, var);
            obs.slot(y, mu, var);
          }
          rep.depth_end(var, (double)m); obs.depth_end(var, (double)m);
        }
        chk_pool_add(pool_rep, rep);
        chk_pool_add(pool_obs, obs);
      }
      // ---- the curve ends: comparison counts and the sums of t_obs / t_rep
#pragma unroll
      for (int code = 0; code < CHK_COUNT; ++code) {
        const double tr = rep.value(code), to = obs.value(code);
        const bool def = !skip && active && tr == tr && to == to;
        const unsigned long long bd = __ballot(def), bge = __ballot(def && tr >= to), bgt = __ballot(def && tr > to);
        if (lane == 0 && bd) {
          atomicAdd(&s_cnt[cj][2][code], __popcll(bd));
          if (bge) atomicAdd(&s_cnt[cj][0][code], __popcll(bge));
          if (bgt) atomicAdd(&s_cnt[cj][1][code], __popcll(bgt));
        }
        const double so = wave_sum(def ? to : 0.0), sr = wave_sum(def ? tr : 0.0);
        if (lane == 0) { s_red[cj][wv][0][code] = so; s_red[cj][wv][1][code] = sr; }
        if (slot >= 0 && active) {
          const size_t o = ((size_t)slot * CHK_COUNT + code) * c.nsets + e;
          c.t_obs[o] = skip ? NAN : to;
          c.t_rep[o] = skip ? NAN : tr;
        }
      }
    }
    if (active) {
      double* pr = c.part + (((size_t)rl * c.tiles + tile) * 2) * CHK_SLOTS * c.nsets + e;
#pragma unroll
      for (int k = 0; k < CHK_SLOTS; ++k) { pr[(size_t)k * c.nsets] = pool_rep[k]; pr[(size_t)(CHK_SLOTS + k) * c.nsets] = pool_obs[k]; }
    }
    __syncthreads();
    for (int x = tid; x < nc * 2 * CHK_COUNT; x += CHK_THREADS) {
      const int cj = x / (2 * CHK_COUNT), k = x % (2 * CHK_COUNT);
      double acc = (&s_sum[cj][0][0])[k];
      for (int w2 = 0; w2 < CHK_WAVES; ++w2) acc += (&s_red[cj][w2][0][0])[k];
      (&s_sum[cj][0][0])[k] = acc;
    }
    __syncthreads();
  }
  // ---- per curve: counts and sums out (nan for a curve without observations and for a bad one)
  const size_t NM = (size_t)a.N * a.M;
  for (int x = tid; x < nc * CHK_COUNT; x += CHK_THREADS) {
    const int cj = x / CHK_COUNT, code = x % CHK_COUNT;
    const size_t curve = (size_t)i * a.M + j0 + cj;
    const bool skip = s_nobs[cj] == 0 || s_bad[cj] != 0;
    double* o = c.cur + (size_t)code * NM + curve;
    const size_t step = (size_t)CHK_COUNT * NM;
    o[CHK_O_GE * step] = skip ? NAN : (double)s_cnt[cj][0][code];
    o[CHK_O_GT * step] = skip ? NAN : (double)s_cnt[cj][1][code];
    o[CHK_O_DEFINED * step] = skip ? NAN : (double)s_cnt[cj][2][code];
    o[CHK_O_SUM_OBS * step] = skip ? NAN : s_sum[cj][0][code];
    o[CHK_O_SUM_REP * step] = skip ? NAN : s_sum[cj][1][code];
    if (code == 0) c.nobs[curve] = skip ? NAN : (double)s_nobs[cj];
  }
}

// tot[2][CHK_SLOTS][nsets] (+)= the partials of the launch's workgroups in index order (rows, then tiles); `first`: the
// first launch of the call starts the sums.  One thread per (side, slot, set): the order is the same for any chunking.
static __global__ void chk_pool_kernel(const double* __restrict__ part, long long nwg, int nsets, int first, double* __restrict__ tot) {
  const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x, per = (long long)2 * CHK_SLOTS * nsets;
  if (x >= per) return;
  const bool is_max = (x / nsets) % CHK_SLOTS == CHK_S_MAX;
  double acc = first ? 0.0 : tot[x];
  for (long long w = 0; w < nwg; ++w) {
    const double v = part[w * per + x];
    acc = is_max ? fmax(acc, v) : acc + v;
  }
  tot[x] = acc;
}

#define BTF_CHK_SET(P, F) P void chk_kernel<F>(ChkArgs);
// instantiated in btf_predict.hip beside the predictive kernels, declared here for the C-ABI unit
#ifndef BTF_PRED_UNIT
#define BTF_X extern template __global__
BTF_CHK_SET(BTF_X, 0) BTF_CHK_SET(BTF_X, 1) BTF_CHK_SET(BTF_X, 2) BTF_CHK_SET(BTF_X, 3) BTF_CHK_SET(BTF_X, 4)
#undef BTF_X
#endif
#endif  // __HIPCC__

}  // namespace btf
