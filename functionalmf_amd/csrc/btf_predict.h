// Posterior predictive of the observations over the kept samples  (btf_predict_eval, btf_predict_batch)
//
// Reference: flutrends/benchmark.py:60-75 (Y_samples ~ N(Mu_hat_s, nu2_s), 2.5 / 97.5 percentiles per cell, :129-134 the
// coverage of the held-out years) and politics/benchmark.py:147-172 (per-sample RMSE / MAE of E[y | theta_s], with
// Mu = R p / (1 - p) for the Negative-Binomial model).  The (S,N,M,T) tensor of draws is never formed: a workgroup takes
// `cells` consecutive (j,t) cells of one row i, draws their n = S x R replicated observations into LDS, and reads the
// moments, the order statistics and the comparisons with the data off the chip's own copy.
//
// Samplers.  Every draw is a pure function of (seed, family stream, global draw index g = (cell S + s) R + r): draw g owns
// the PRED_BLOCKS Philox blocks [g PRED_BLOCKS, (g + 1) PRED_BLOCKS) of its stream (a draw that needed more - below
// 1e-40 - moves to the next stream), so the result does not depend on the launch geometry, on which cells are asked
// for or on where W, V come from.
//   normal     eta + sqrt(v) philox_normal(seed, stream, g)
//   Poisson    lam < 10: inversion by sequential search (one uniform); else Hoermann's PTRS (transformed rejection with
//              squeeze, 1993; numpy's algorithm), the acceptance test in a cancellation-free form
//                log f(k) = d - k log1p(d / lam) - log(2 pi (k + 1)) / 2 - fc(k),   d = k + 1 - lam,
//              fc the Stirling tail of log k! (table for k <= 9, four series terms above: < 1e-13)
//   Binomial   n min(p, 1-p) < 10: inversion (BINV); else Hoermann's BTRS (1993) with the same tail; p > 1/2 by symmetry
//   NegBin     Poisson with rate Gamma(r) exp(eta): Marsaglia & Tsang (2000) on this generator
// Every rejection loop is flat: one candidate per trip and lane, lanes that are done idle; the inversion search, the
// gamma loop and the transformed-rejection loop follow each other, none is nested in another.
//
// The samplers are __host__ __device__ so that the host can restate a draw (tests of the counter layout).
#pragma once
#include "btf_device.h"
#include <math.h>

namespace btf {

enum { PRED_FAM_POISSON_LOG = 0, PRED_FAM_POISSON_IDENTITY = 1, PRED_FAM_LOGIT = 2, PRED_FAM_GAUSSIAN = 3, PRED_FAM_NEGBIN = 4,
       PRED_FAM_COUNT = 5,                     // the families of btf_predict_eval
       PRED_FAM_GAMMA_GRID = 5 };              // the table family of btf_gg_predict.h, behind entry points of its own
constexpr int PRED_BLOCKS = 64;                 // Philox blocks reserved per draw
constexpr double PRED_POIS_SWITCH = 10.0;       // Poisson: inversion below, PTRS from here
constexpr double PRED_BINOM_SWITCH = 10.0;      // Binomial: inversion while n min(p,1-p) is below, BTRS from here
constexpr int PRED_MAX_DRAWS = 16384;           // S x R per cell (LDS)
constexpr int PRED_THREADS = 256;
constexpr unsigned long long PRED_STREAM = 0x7072656469637400ULL;     // + family; spill streams: + (ctr / PRED_BLOCKS) << 8

struct PredRng {
  unsigned long long seed, stream, base;
  unsigned ctr;
  __host__ __device__ PredRng(unsigned long long seed_, int family, unsigned long long g)
      : seed(seed_), stream(PRED_STREAM + (unsigned long long)family), base(g * (unsigned long long)PRED_BLOCKS), ctr(0) {}
  __host__ __device__ inline void uniform2(double& u, double& v) {
    uint32_t r[4];
    Philox::gen(seed, stream + ((unsigned long long)(ctr / PRED_BLOCKS) << 8), base + (ctr % PRED_BLOCKS), r);
    ++ctr;
    u = u01(r[0], r[1]);
    v = u01(r[2], r[3]);
  }
};

// log k! = (k + 1/2) log(k + 1) - (k + 1) + log(2 pi) / 2 + fc(k)
__host__ __device__ inline double pred_fc(double k) {
  if (k < 10.0) {
    switch ((int)k) {
      case 0: return 0.08106146679532726;
      case 1: return 0.04134069595540929;
      case 2: return 0.02767792568499834;
      case 3: return 0.02079067210376509;
      case 4: return 0.01664469118982119;
      case 5: return 0.01387612882307075;
      case 6: return 0.01189670994589177;
      case 7: return 0.01041126526197209;
      case 8: return 0.009255462182712733;
      default: return 0.008330563433362871;
    }
  }
  const double x = 1.0 / (k + 1.0), x2 = x * x;
  return x * (1.0 / 12.0 - x2 * (1.0 / 360.0 - x2 * (1.0 / 1260.0 - x2 * (1.0 / 1680.0))));
}

__host__ __device__ inline double pred_poisson(double lam, PredRng& g) {
  if (lam == 0.0) return 0.0;
  if (!(lam > 0.0 && lam < INFINITY)) return NAN;
  double k = 0.0;
  if (lam < PRED_POIS_SWITCH) {
    double u, spare;
    g.uniform2(u, spare);
    double p = exp(-lam);
    while (u > p && k < 1000.0) {                 // (the cap: u within rounding of 1)
      u -= p;
      k += 1.0;
      p *= lam / k;
    }
    return k;
  }
  const double slam = sqrt(lam), b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
  const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
  bool go = true;
  while (go) {
    double U, V;
    g.uniform2(U, V);
    U -= 0.5;
    const double us = 0.5 - fabs(U);
    const double kk = floor((2.0 * a / us + b) * U + lam + 0.43);
    if (us >= 0.07 && V <= vr) { k = kk; go = false; }
    else if (kk < 0.0 || (us < 0.013 && V > us)) { }
    else {
      const double d = kk + 1.0 - lam;
      const double lf = d - kk * log1p(d / lam) - 0.5 * log(6.283185307179586 * (kk + 1.0)) - pred_fc(kk);
      if (log(V * invalpha / (a / (us * us) + b)) <= lf) { k = kk; go = false; }
    }
  }
  return k;
}

// Binomial(n, p), p given as eta = logit(p) (both tails exact: min(p, 1-p) = 1 / (1 + exp(|eta|)))
__host__ __device__ inline double pred_binomial(double n, double eta, PredRng& g) {
  if (!(n >= 0.0 && n < INFINITY) || n != floor(n) || eta != eta) return NAN;
  if (n == 0.0) return 0.0;
  const bool flip = eta > 0.0;
  const double e = exp(-fabs(eta));               // odds of the smaller side: r = p / q
  const double p = e / (1.0 + e), q = 1.0 / (1.0 + e);
  double k = 0.0;
  if (n * p < PRED_BINOM_SWITCH) {
    double u, spare;
    g.uniform2(u, spare);
    double f = exp(n * log1p(-p));                // q^n
    const double a = (n + 1.0) * e;
    while (u > f && k < n) {
      u -= f;
      k += 1.0;
      f *= a / k - e;
    }
  } else {
    const double spq = sqrt(n * p * q), b = 1.15 + 2.53 * spq, a = -0.0873 + 0.0248 * b + 0.01 * p, c = n * p + 0.5;
    const double vr = 0.92 - 4.2 / b, alpha = (2.83 + 5.1 / b) * spq, m = floor((n + 1.0) * p);
    const double hm = (m + 0.5) * log((m + 1.0) / (e * (n - m + 1.0))) + pred_fc(m) + pred_fc(n - m);
    bool go = true;
    while (go) {
      double U, V;
      g.uniform2(U, V);
      U -= 0.5;
      const double us = 0.5 - fabs(U);
      const double kk = floor((2.0 * a / us + b) * U + c);
      if (us >= 0.07 && V <= vr) { k = kk; go = false; }
      else if (kk < 0.0 || kk > n) { }
      else {
        const double nk = n - kk + 1.0;
        const double ub = hm + (n + 1.0) * log1p((kk - m) / nk) + (kk + 0.5) * log(e * nk / (kk + 1.0)) - pred_fc(kk) - pred_fc(n - kk);
        if (log(V * alpha / (a / (us * us) + b)) <= ub) { k = kk; go = false; }
      }
    }
  }
  return flip ? n - k : k;
}

__host__ __device__ inline double pred_unit_normal(double u1, double u2) {
  const double rad = sqrt(-2.0 * log(u1));
#ifdef __HIP_DEVICE_COMPILE__
  return rad * cospi(2.0 * u2);
#else
  return rad * cos(6.283185307179586 * u2);
#endif
}

// Gamma(shape, 1), Marsaglia & Tsang; shape < 1 by the U^(1/shape) boost.  Two Philox blocks per candidate.
__host__ __device__ inline double pred_gamma(double shape, PredRng& g) {
  if (!(shape > 0.0 && shape < INFINITY)) return NAN;
  double boost = 1.0;
  if (shape < 1.0) {
    double u, spare;
    g.uniform2(u, spare);
    boost = exp(log(u) / shape);
    shape += 1.0;
  }
  const double d = shape - 1.0 / 3.0, cc = 1.0 / sqrt(9.0 * d);
  double out = 0.0;
  bool go = true;
  while (go) {
    double u1, u2, u3, spare;
    g.uniform2(u1, u2);
    g.uniform2(u3, spare);
    const double x = pred_unit_normal(u1, u2);
    double v = 1.0 + cc * x;
    if (v > 0.0) {
      v = v * v * v;
      const double x2 = x * x;
      if (u3 < 1.0 - 0.0331 * x2 * x2 || log(u3) < 0.5 * x2 + d * (1.0 - v + log(v))) { out = d * v; go = false; }
    }
  }
  return boost * out;
}

// E[y | eta, aux]: aux = trials (logit), the rate r (Negative-Binomial); unused otherwise
template <int FAM>
__host__ __device__ inline double pred_mean(double eta, double aux) {
  if constexpr (FAM == PRED_FAM_POISSON_LOG) return exp(eta);
  else if constexpr (FAM == PRED_FAM_POISSON_IDENTITY) return eta > 0.0 ? eta : NAN;
  else if constexpr (FAM == PRED_FAM_LOGIT) return aux / (1.0 + exp(-eta));
  else if constexpr (FAM == PRED_FAM_GAUSSIAN) return eta;
  else return aux * exp(eta);
}

#ifdef __HIPCC__
// draw number g of y | eta, aux (aux: trials / variance / rate); tab, G: the table of a family that has one (pred_stage)
template <int FAM>
__device__ inline double pred_draw(double eta, double aux, unsigned long long seed, unsigned long long g,
                                   const double* tab = nullptr, int G = 0) {
  if constexpr (FAM == PRED_FAM_GAUSSIAN) {
    return aux >= 0.0 ? fma(sqrt(aux), philox_normal(seed, PRED_STREAM + FAM, g), eta) : NAN;
  } else {
    PredRng rng(seed, FAM, g);
    if constexpr (FAM == PRED_FAM_POISSON_LOG) return pred_poisson(exp(eta), rng);
    else if constexpr (FAM == PRED_FAM_POISSON_IDENTITY) return eta > 0.0 ? pred_poisson(eta, rng) : NAN;
    else if constexpr (FAM == PRED_FAM_LOGIT) return pred_binomial(aux, eta, rng);
    else {
      const double lam = pred_gamma(aux, rng) * exp(eta);
      return pred_poisson(lam, rng);
    }
  }
}

template <int FAM>
__global__ __launch_bounds__(PRED_THREADS) void pred_batch_kernel(const double* __restrict__ eta, const double* __restrict__ aux,
                                                                 long long n, unsigned long long seed, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * PRED_THREADS + threadIdx.x;
  if (i < n) out[i] = pred_draw<FAM>(eta[i], aux[i], seed, (unsigned long long)i);
}

struct PredArgs {
  const double* W;                       // [S][N][K]
  const double* V;                       // [S][M][T][K]
  const double* aux; long long aux_stride;   // per-sample parameter: aux[s * stride + rate index], or null: par
  int aux_n0, aux_n1, aux_n2;            // the rate's extent along rows / columns / depth (1: shared), Gaussian: 1,1,1
  double par;                            // Gaussian: the variance, Negative-Binomial: the rate (when aux is null)
  const double* trials;                  // [N][M][T] or null (1 trial)
  const double* Y; int nreps;            // [N][M][T][nreps] or null
  int S, R, N, M, T, K;
  int P, cells;                          // LDS row length (power of two >= S R), cells per workgroup
  unsigned long long seed;
  const double* q; int nq;
  const int* list; int nlist;            // cells whose draws are written out
  double *mean, *y_mean, *y_var, *quant, *pit_lo, *pit_hi, *inside, *nobs, *draws;     // any may be null
  double *score_part;                    // [2][S][chunks] + counts [chunks]: pred_score_kernel
  int chunks;
  const double* gg; int gg_G;            // gamma grid: the table [a | s | c] of gg_pred_table (par: mbar)
};

// The table of a family that draws from one, staged in LDS by every thread of the workgroup before the first draw
// (btf_gg_predict.h specialises it); null: the family has none.
template <int FAM>
__device__ __forceinline__ const double* pred_stage(const PredArgs&) { return nullptr; }

template <int FAM>
__device__ __forceinline__ double pred_aux(const PredArgs& a, int s, int i, int j, int t) {
  if constexpr (FAM == PRED_FAM_LOGIT) return a.trials ? a.trials[((size_t)i * a.M + j) * a.T + t] : 1.0;
  else if constexpr (FAM == PRED_FAM_GAUSSIAN || FAM == PRED_FAM_NEGBIN) {
    if (!a.aux) return a.par;
    const size_t ri = ((size_t)(a.aux_n0 > 1 ? i : 0) * a.aux_n1 + (a.aux_n1 > 1 ? j : 0)) * a.aux_n2 + (a.aux_n2 > 1 ? t : 0);
    return a.aux[(size_t)s * a.aux_stride + ri];
  } else return 0.0;
}

__device__ __forceinline__ double pred_eta(const PredArgs& a, int s, int i, int jt) {
  const double* __restrict__ w = a.W + ((size_t)s * a.N + i) * a.K;
  const double* __restrict__ v = a.V + ((size_t)s * a.M * a.T + jt) * a.K;
  double x = 0.0;
  for (int k = 0; k < a.K; ++k) x = fma(w[k], v[k], x);
  return x;
}

// One workgroup: row i = blockIdx.x % N (fastest: the workgroups in flight share their V slices), cells jt0 .. jt0 + cells.
template <int FAM>
__global__ __launch_bounds__(PRED_THREADS) void pred_kernel(PredArgs a) {
  extern __shared__ double srt[];                 // [cells][P]
  const int i = blockIdx.x % a.N, MT = a.M * a.T, jt0 = (blockIdx.x / a.N) * a.cells;
  const int nc = min(a.cells, MT - jt0), n = a.S * a.R, P = a.P, cells = a.cells;
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const double* tab = pred_stage<FAM>(a);
  // ---- draws: thread -> (cell c, draw d = s R + r), c fastest (V[s][jt0 + c][:] is contiguous over c)
  for (int e = threadIdx.x; e < cells * P; e += PRED_THREADS) {
    const int c = e % cells, d = e / cells;
    double val = __builtin_inf();
    if (d < n && c < nc) {
      const int s = d / a.R, jt = jt0 + c;
      const double eta = pred_eta(a, s, i, jt);
      const unsigned long long cell = (unsigned long long)i * MT + jt;
      val = pred_draw<FAM>(eta, pred_aux<FAM>(a, s, i, jt / a.T, jt % a.T), a.seed, cell * (unsigned long long)n + d, tab, a.gg_G);
    }
    srt[(size_t)c * P + d] = val;
  }
  __syncthreads();
  // ---- the raw draws of the listed cells, in draw order (before the sort)
  if (a.draws) {
    for (int c = wv; c < nc; c += PRED_THREADS / WAVE) {
      const int flat = i * MT + jt0 + c;
      for (int l0 = 0; l0 < a.nlist; l0 += WAVE) {
        const int li = l0 + lane;
        unsigned long long hit = __ballot(li < a.nlist && a.list[li] == flat);
        while (hit) {
          const int b = __builtin_ctzll(hit);
          hit &= hit - 1;
          double* dst = a.draws + (size_t)(l0 + b) * n;
          for (int d = lane; d < n; d += WAVE) dst[d] = srt[(size_t)c * P + d];
        }
      }
    }
    __syncthreads();
  }
  // ---- bitonic sort of every row (ascending); P/2 compare-exchanges per row and stage
  const int half = P >> 1;
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int e = threadIdx.x; e < cells * half; e += PRED_THREADS) {
        const int c = e / half, pidx = e - c * half;
        const int i1 = ((pidx / jj) * 2 * jj) + (pidx % jj), i2 = i1 + jj;
        double* row = srt + (size_t)c * P;
        const double x = row[i1], y = row[i2];
        const bool up = (i1 & kk) == 0;
        if ((x > y) == up) { row[i1] = y; row[i2] = x; }
      }
      __syncthreads();
    }
  }
  // ---- per cell, one wave: lanes stride over the draws / samples, partial sums meet in a fixed butterfly
  for (int c = wv; c < nc; c += PRED_THREADS / WAVE) {
    const double* row = srt + (size_t)c * P;
    const int jt = jt0 + c, j = jt / a.T, t = jt % a.T;
    const size_t o = (size_t)i * MT + jt;
    if (a.mean) {
      double sm = 0.0;
      for (int s = lane; s < a.S; s += WAVE) sm += pred_mean<FAM>(pred_eta(a, s, i, jt), pred_aux<FAM>(a, s, i, j, t));
      sm = wave_sum(sm);
      if (lane == 0) a.mean[o] = sm / a.S;
    }
    double sum = 0.0;
    for (int d = lane; d < n; d += WAVE) sum += row[d];
    const double ym = wave_sum(sum) / n;
    const bool bad = ym != ym;                      // a nan draw (missing trials, eta <= 0 under the identity link)
    if (a.y_mean && lane == 0) a.y_mean[o] = ym;
    if (a.y_var) {
      double ss = 0.0;
      for (int d = lane; d < n; d += WAVE) { const double r = row[d] - ym; ss = fma(r, r, ss); }
      ss = wave_sum(ss);
      if (lane == 0) a.y_var[o] = n > 1 ? ss / (n - 1) : NAN;
    }
    double qlo = NAN, qhi = NAN;
    for (int q0 = 0; q0 < a.nq; q0 += WAVE) {
      const int qi = min(q0 + lane, a.nq - 1);
      const double pos = a.q[qi] / 100.0 * (n - 1);
      int lo = (int)floor(pos);
      lo = max(0, min(lo, n - 1));
      const int hi = min(lo + 1, n - 1);
      const double val = bad ? NAN : row[lo] + (pos - lo) * (row[hi] - row[lo]);
      if (a.quant && q0 + lane < a.nq) a.quant[(size_t)qi * a.N * MT + o] = val;
      if (q0 == 0) qlo = bcast_lane(val, 0);
      if (q0 + WAVE >= a.nq) qhi = bcast_lane(val, (a.nq - 1) - q0);
    }
    if (a.Y) {
      double lt = 0.0, le = 0.0, in = 0.0, no = 0.0;
      for (int r = 0; r < a.nreps; ++r) {
        const double y = a.Y[o * a.nreps + r];
        if (y != y) continue;                       // wave-uniform
        int clt = 0, cle = 0;
        for (int d = lane; d < n; d += WAVE) { clt += row[d] < y; cle += row[d] <= y; }
        lt += (double)clt; le += (double)cle;
        no += 1.0;
        in += (qlo <= y && y <= qhi) ? 1.0 : 0.0;
      }
      lt = wave_sum(lt); le = wave_sum(le);         // (integers below 2^53: exact in any order)
      if (lane == 0) {
        const double den = (double)n * no;
        if (a.pit_lo) a.pit_lo[o] = (no > 0.0 && !bad) ? lt / den : NAN;
        if (a.pit_hi) a.pit_hi[o] = (no > 0.0 && !bad) ? le / den : NAN;
        if (a.inside) a.inside[o] = (a.nq >= 2 && !bad) ? in : NAN;
        if (a.nobs) a.nobs[o] = no;
      }
    }
  }
}

// Per-sample squared and absolute error of E[y | theta_s] over the observed y: workgroup (chunk, s) takes PRED_SCORE_CELLS
// consecutive cells, its threads stride over them, the partial sums meet in a fixed order; pred_score_total_kernel adds
// the chunks in chunk order.
constexpr int PRED_SCORE_CELLS = 4096;
template <int FAM>
__global__ __launch_bounds__(PRED_THREADS) void pred_score_kernel(PredArgs a) {
  __shared__ double red[3][PRED_THREADS / WAVE];
  const int s = blockIdx.y, ch = blockIdx.x, MT = a.M * a.T;
  const long long ncell = (long long)a.N * MT;
  const long long c0 = (long long)ch * PRED_SCORE_CELLS, c1 = c0 + PRED_SCORE_CELLS < ncell ? c0 + PRED_SCORE_CELLS : ncell;
  double se = 0.0, ae = 0.0, cnt = 0.0;
  for (long long c = c0 + threadIdx.x; c < c1; c += PRED_THREADS) {
    const int i = (int)(c / MT), jt = (int)(c % MT);
    double mu = 0.0;
    bool have = false;
    for (int r = 0; r < a.nreps; ++r) {
      const double y = a.Y[(size_t)c * a.nreps + r];
      if (y != y) continue;
      if (!have) { mu = pred_mean<FAM>(pred_eta(a, s, i, jt), pred_aux<FAM>(a, s, i, jt / a.T, jt % a.T)); have = true; }
      const double rres = y - mu;
      se = fma(rres, rres, se);
      ae += fabs(rres);
      cnt += 1.0;
    }
  }
  se = wave_sum(se); ae = wave_sum(ae); cnt = wave_sum(cnt);
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  if (lane == 0) { red[0][wv] = se; red[1][wv] = ae; red[2][wv] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    for (int w = 0; w < PRED_THREADS / WAVE; ++w) { x0 += red[0][w]; x1 += red[1][w]; x2 += red[2][w]; }
    a.score_part[((size_t)0 * a.S + s) * a.chunks + ch] = x0;
    a.score_part[((size_t)1 * a.S + s) * a.chunks + ch] = x1;
    a.score_part[((size_t)2 * a.S + s) * a.chunks + ch] = x2;
  }
}

// out[0][s] = rmse, out[1][s] = mae
static __global__ void pred_score_total_kernel(const double* __restrict__ part, int S, int chunks, double* __restrict__ out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  double se = 0.0, ae = 0.0, cnt = 0.0;
  for (int c = 0; c < chunks; ++c) {
    se += part[((size_t)0 * S + s) * chunks + c];
    ae += part[((size_t)1 * S + s) * chunks + c];
    cnt += part[((size_t)2 * S + s) * chunks + c];
  }
  out[s] = cnt > 0.0 ? sqrt(se / cnt) : NAN;
  out[S + s] = cnt > 0.0 ? ae / cnt : NAN;
}

#define BTF_PRED_SET(P, F)                                                                                        \
  P void pred_batch_kernel<F>(const double*, const double*, long long, unsigned long long, double*);              \
  P void pred_kernel<F>(PredArgs); P void pred_score_kernel<F>(PredArgs);

// instantiated in btf_predict.hip (its own compilation unit), declared here for the C-ABI unit
#ifndef BTF_PRED_UNIT
#define BTF_X extern template __global__
BTF_PRED_SET(BTF_X, 0) BTF_PRED_SET(BTF_X, 1) BTF_PRED_SET(BTF_X, 2) BTF_PRED_SET(BTF_X, 3) BTF_PRED_SET(BTF_X, 4)
#undef BTF_X
#endif
#endif  // __HIPCC__

}  // namespace btf
