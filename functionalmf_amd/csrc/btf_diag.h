// Convergence diagnostics per cell of Mu = W V': split R-hat, bulk / tail ESS and the MCSE of the mean  (btf_diag_eval)
//
// Definition: Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021), "Rank-normalization, folding, and localization",
// as functionalmf_amd/diagnostics.py states it in numpy (chain_diagnostics), with one chain allowed (its two halves).
// Per cell (i, jt) the series is x[c][s] = f(w_i^(c,s) . v_jt^(c,s)) over C chains of S draws; the (C, S, N, M, T)
// tensor is never formed.  W and V are identified only up to rotation and sign, so the cells of W V' are what can be
// checked, not factor entries.
//
// Geometry: one workgroup of DIAG_THREADS per cell; cells are numbered row-fastest (cell = jt * N + i), so the
// workgroups in flight share jt and read the same v_jt^(c,s) lines.  LDS holds the draws twice:
//   X[c*S + s]  the values in draw order (the raw series and the tail indicators read it)
//   B[P]        the values sorted once (bitonic, padded to a power of two with +inf); later the z-scores in split order
// From the sorted row: the median and numpy's 'linear' q05 / q95.  Average ranks over the split draws come from two
// binary searches per draw (lower and upper bound), less the middle draws an odd S drops.  The rank of |x - median| among
// the folded draws is the count in a window around the median: |B[j] - m| is non-increasing left of the median and
// non-decreasing right of it (rounding is monotone), so two binary searches on each side give it without a second sort.
// z = Phi^-1((r - 3/8) / (n + 1/4)) with Wichura's AS241 (fp64, ~1e-16 relative).  The z-scores of a thread's draws stay
// in registers (DIAG_PER each) until the sorted row is no longer needed.
//
// ESS: autocovariances are direct sums over lags, two lags per pass, for four series at once (bulk z, the two tail
// indicators, the raw draws for the MCSE); each series follows Geyer's initial positive sequence and stops on its own,
// the monotone step is applied online as the pairs are accepted.  Every sum has a fixed order (strided per-thread sums,
// butterfly within a wave, waves in order): two calls agree bit for bit.  No floating-point atomics.
//
// A cell whose draws are all equal, or hold a non-finite value, gets nan in every output.
#pragma once
#include "btf_device.h"
#include <math.h>

namespace btf {

constexpr int DIAG_THREADS = 256;
constexpr int DIAG_WAVES = DIAG_THREADS / WAVE;
constexpr int DIAG_MAX_DRAWS = 4096;                            // pooled C * S per cell (LDS: 2 x 32 KiB)
constexpr int DIAG_MAX_CHAINS = 64;
constexpr int DIAG_PER = DIAG_MAX_DRAWS / DIAG_THREADS;          // split draws per thread
constexpr int DIAG_OUT = 5;                                      // rhat, ess_bulk, ess_tail, mcse_mean, mean

struct DiagArgs {
  const double* const* W;      // [C] -> [S][N][K]
  const double* const* V;      // [C] -> [S][MT][K]
  int C, S, N, MT, P, transform;
  double* out;                 // [DIAG_OUT][N][MT]
};

// Wichura (1988), AS241 PPND16: the standard normal quantile, ~1e-16 relative
__host__ __device__ inline double diag_ppf(double p) {
  const double q = p - 0.5;
  double r, val;
  if (fabs(q) <= 0.425) {
    r = 0.180625 - q * q;
    val = q * (((((((r * 2509.0809287301226727 + 33430.575583588128105) * r + 67265.770927008700853) * r +
                   45921.953931549871457) * r + 13731.693765509461125) * r + 1971.5909503065514427) * r +
                133.14166789178437745) * r + 3.387132872796366608) /
          (((((((r * 5226.495278852545925 + 28729.085735721942674) * r + 39307.89580009271061) * r +
               21213.794301586595867) * r + 5394.1960214247511077) * r + 687.1870074920579083) * r +
            42.313330701600911252) * r + 1.0);
    return val;
  }
  r = q < 0 ? p : 1.0 - p;
  r = sqrt(-log(r));
  if (r <= 5.0) {
    r -= 1.6;
    val = (((((((r * 7.7454501427834140764e-4 + 0.0227238449892691845833) * r + 0.24178072517745061177) * r +
                1.27045825245236838258) * r + 3.64784832476320460504) * r + 5.7694972214606914055) * r +
             4.6303378461565452959) * r + 1.42343711074968357734) /
          (((((((r * 1.05075007164441684324e-9 + 5.475938084995344946e-4) * r + 0.0151986665636164571966) * r +
                0.14810397642748007459) * r + 0.68976733498510000455) * r + 1.6763848301838038494) * r +
             2.05319162663775882187) * r + 1.0);
  } else {
    r -= 5.0;
    val = (((((((r * 2.01033439929228813265e-7 + 2.71155556874348757815e-5) * r + 0.0012426609473880784386) * r +
                0.026532189526576123093) * r + 0.29656057182850489123) * r + 1.7848265399172913358) * r +
             5.4637849111641143699) * r + 6.6579046435011037772) /
          (((((((r * 2.04426310338993978564e-15 + 1.4215117583164458887e-7) * r + 1.8463183175100546818e-5) * r +
                7.868691311456132591e-4) * r + 0.0148753612908506148525) * r + 0.13692988092273580531) * r +
             0.59983220655588793769) * r + 1.0);
  }
  return q < 0.0 ? -val : val;
}

// sums of NV per-thread values over the workgroup, every thread gets them; fixed order
template <int NV>
__device__ __forceinline__ void diag_block_sum(double (&v)[NV], double (*red)[DIAG_WAVES]) {
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = wave_sum(v[q]);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < NV; ++q) red[q][wv] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < DIAG_WAVES; ++w) t += red[q][w];
    v[q] = t;
  }
  __syncthreads();
}

// per split chain q < nq (nq <= 2 DIAG_MAX_CHAINS): out[v][q] = sum over k < h of f(q, k)[v]; fixed order
template <int NV, class F>
__device__ __forceinline__ void diag_seg_sum(int nq, int h, F f, double (*out)[2 * DIAG_MAX_CHAINS], double (*red)[DIAG_WAVES]) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  int G = DIAG_THREADS / nq;
  G = 1 << (31 - __builtin_clz(G));                       // threads per chain, a power of two >= 2
  const int q = tid / G, sub = tid & (G - 1);
  double acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.0;
  if (q < nq) {
    for (int k = sub; k < h; k += G) {
      double t[NV];
      f(q, k, t);
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[v] += t[v];
    }
  }
  const int Gw = G < WAVE ? G : WAVE;
  for (int off = Gw >> 1; off > 0; off >>= 1) {
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] += __shfl_xor(acc[v], off, WAVE);
  }
  if (G <= WAVE) {
    if (sub == 0 && q < nq) {
#pragma unroll
      for (int v = 0; v < NV; ++v) out[v][q] = acc[v];
    }
  } else {
    if (lane == 0) {
#pragma unroll
      for (int v = 0; v < NV; ++v) red[v][wv] = acc[v];
    }
    __syncthreads();
    if (tid < nq) {
      const int per = G / WAVE;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        double t = 0.0;
        for (int w = 0; w < per; ++w) t += red[v][tid * per + w];
        out[v][tid] = t;
      }
    }
  }
  __syncthreads();
}

// first index in [lo, hi) of the sorted row with row[j] >= x (strict: > x)
template <bool STRICT>
__device__ __forceinline__ int diag_bound(const double* row, int lo, int hi, double x) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const bool right = STRICT ? row[mid] > x : row[mid] >= x;
    if (right) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// left of the median (|row - m| non-increasing): first index in [lo, hi) with |row[j] - m| <= d (strict: < d)
template <bool STRICT>
__device__ __forceinline__ int diag_fold_left(const double* row, int lo, int hi, double m, double d) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const double g = fabs(row[mid] - m);
    if (STRICT ? g < d : g <= d) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// right of the median (|row - m| non-decreasing): first index in [lo, hi) with |row[j] - m| > d (strict: >= d)
template <bool STRICT>
__device__ __forceinline__ int diag_fold_right(const double* row, int lo, int hi, double m, double d) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const double g = fabs(row[mid] - m);
    if (STRICT ? g >= d : g > d) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// numpy 'linear' quantile of a sorted row of n values (np.quantile: index (n - 1) q, _lerp)
__device__ __forceinline__ double diag_quantile(const double* row, int n, double q) {
  const double vi = (n - 1) * q;
  if (vi >= n - 1) return row[n - 1];
  const double fl = floor(vi);
  const int lo = (int)fl;
  const double t = vi - fl, a = row[lo], b = row[lo + 1];
  const double diff = b - a;
  return t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
}

// Geyer's initial positive sequence, fed two lags at a time; the monotone step is applied online
struct DiagGeyer {
  double mean_var, var_plus, even, odd, prev, main, pend, last_even;
  int iters;
  bool active, last_acc;
  __device__ void start(double acov0, double acov1, double chain_mean_var, int h) {   // acov: means over the chains
    mean_var = acov0 * h / (h - 1);
    var_plus = mean_var * (h - 1) / h + chain_mean_var;
    even = 1.0;
    odd = 1.0 - (mean_var - acov1) / var_plus;
    prev = even + odd;
    main = prev;
    iters = 0;
    last_acc = false;
    last_even = 0.0;
    pend = 0.0;
  }
  __device__ bool wants(int t, int h) const { return t < h - 3 && even + odd > 0.0; }
  __device__ void feed(double acov_a, double acov_b) {
    if (iters > 0) {                                      // the previous pair was accepted and is not the last: commit
      double p = pend;
      if (p > prev) p = prev;
      main += p;
      prev = p;
    }
    even = 1.0 - (mean_var - acov_a) / var_plus;
    odd = 1.0 - (mean_var - acov_b) / var_plus;
    last_acc = even + odd >= 0.0;
    pend = even + odd;
    last_even = even;
    ++iters;
  }
  __device__ double ess(int nq, int h) const {
    double tau;
    if (iters == 0) tau = 0.0;                            // -1 + rho[0]
    else tau = -1.0 + 2.0 * main + ((last_acc || last_even > 0.0) ? last_even : 0.0);
    const double lim = 1.0 / log10((double)nq * h);
    if (lim > tau) tau = lim;
    return (double)nq * h / tau;
  }
};

template <int K>
__global__ __launch_bounds__(DIAG_THREADS) void diag_kernel(DiagArgs a) {
  extern __shared__ double lds[];
  __shared__ double cm[4][2 * DIAG_MAX_CHAINS];           // per split chain: means of the four series
  __shared__ double red[8][DIAG_WAVES];
  const int C = a.C, S = a.S, n = C * S, h = S / 2, nq = 2 * C, ns = nq * h, P = a.P, N = a.N, MT = a.MT;
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const int i = (int)(cell % N), jt = (int)(cell / N);
  const size_t cells = (size_t)N * MT, oc = (size_t)i * MT + jt;
  double* X = lds;               // [n]
  double* B = lds + n;           // [P]
  // ---- the values: draw e = c * S + s
  int bad = 0;
  for (int e = tid; e < P; e += DIAG_THREADS) {
    double x = __builtin_inf();
    if (e < n) {
      const int c = e / S, s = e - c * S;
      const double* __restrict__ w = a.W[c] + ((size_t)s * N + i) * K;
      const double* __restrict__ v = a.V[c] + ((size_t)s * MT + jt) * K;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) acc = fma(w[k], v[k], acc);
      x = a.transform == 1 ? 1.0 / (1.0 + exp(-acc)) : (a.transform == 2 ? acc * acc : acc);
      bad |= !isfinite(x);
      X[e] = x;
    }
    B[e] = x;
  }
  bad = __syncthreads_or(bad);
  if (bad) {
    if (tid < DIAG_OUT) a.out[tid * cells + oc] = __builtin_nan("");
    return;
  }
  // ---- bitonic sort of B (ascending)
  const int half = P >> 1;
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int e = tid; e < half; e += DIAG_THREADS) {
        const int i1 = ((e / jj) * 2 * jj) + (e % jj), i2 = i1 + jj;
        const double x1 = B[i1], x2 = B[i2];
        const bool up = (i1 & kk) == 0;
        if ((x1 > x2) == up) { B[i1] = x2; B[i2] = x1; }
      }
      __syncthreads();
    }
  }
  if (B[0] == B[n - 1]) {                                 // every draw equal
    if (tid < DIAG_OUT) a.out[tid * cells + oc] = __builtin_nan("");
    return;
  }
  const double med = (n & 1) ? B[n / 2] : (B[n / 2 - 1] + B[n / 2]) / 2.0;
  const double q05 = diag_quantile(B, n, 0.05), q95 = diag_quantile(B, n, 0.95);
  const int L = diag_bound<false>(B, 0, n, med);          // B[j] < med for j < L
  const bool odd_s = (S & 1) != 0;                        // the middle draw s = h of every chain is dropped by the split
  // ---- z-scores of the split draws (split order: q < C first halves, then second halves; e = q * h + k)
  double zb[DIAG_PER], zf[DIAG_PER];
#pragma unroll
  for (int u = 0; u < DIAG_PER; ++u) {
    const int e = tid + u * DIAG_THREADS;
    zb[u] = 0.0; zf[u] = 0.0;
    if (e < ns) {
      const int q = e / h, k = e - q * h;
      const int c = q < C ? q : q - C;
      const double x = X[c * S + (q < C ? 0 : S - h) + k];
      int lo = diag_bound<false>(B, 0, n, x), hi = diag_bound<true>(B, lo, n, x);
      const double d = fabs(x - med);
      int le = (L - diag_fold_left<false>(B, 0, L, med, d)) + (diag_fold_right<false>(B, L, n, med, d) - L);
      int lt = (L - diag_fold_left<true>(B, 0, L, med, d)) + (diag_fold_right<true>(B, L, n, med, d) - L);
      if (odd_s) {
        for (int c2 = 0; c2 < C; ++c2) {
          const double xd = X[c2 * S + h], dd = fabs(xd - med);
          lo -= xd < x; hi -= xd <= x;
          le -= dd <= d; lt -= dd < d;
        }
      }
      const double rb = 0.5 * (double)(lo + hi + 1), rf = 0.5 * (double)(lt + le + 1);
      zb[u] = diag_ppf((rb - 0.375) / ((double)ns + 0.25));
      zf[u] = diag_ppf((rf - 0.375) / ((double)ns + 0.25));
    }
  }
  __syncthreads();                                        // the sorted row is no longer read
  // ---- folded R-hat
#pragma unroll
  for (int u = 0; u < DIAG_PER; ++u) {
    const int e = tid + u * DIAG_THREADS;
    if (e < ns) B[e] = zf[u];
  }
  __syncthreads();
  diag_seg_sum<1>(nq, h, [&](int q, int k, double (&t)[1]) { t[0] = B[q * h + k]; }, cm, red);
  double rhat_f;
  {
    double ss[1] = {0.0};
    for (int e = tid; e < ns; e += DIAG_THREADS) {
      const int q = e / h;
      const double y = B[e] - cm[0][q] / h;
      ss[0] = fma(y, y, ss[0]);
    }
    diag_block_sum<1>(ss, red);
    double mu = 0.0;
    for (int q = 0; q < nq; ++q) mu += cm[0][q] / h;
    mu /= nq;
    double vb = 0.0;
    for (int q = 0; q < nq; ++q) { const double y = cm[0][q] / h - mu; vb = fma(y, y, vb); }
    const double Bv = h * (vb / (nq - 1)), Wv = ss[0] / (h - 1) / nq;
    rhat_f = sqrt((Bv / Wv + h - 1) / h);
  }
  __syncthreads();                                        // (cm is rewritten below)
  // ---- bulk z into B; per split chain means of the four series
#pragma unroll
  for (int u = 0; u < DIAG_PER; ++u) {
    const int e = tid + u * DIAG_THREADS;
    if (e < ns) B[e] = zb[u];
  }
  __syncthreads();
  auto xoff = [&](int q) { return (q < C ? q * S : (q - C) * S + S - h); };   // X index of the split chain's first draw
  diag_seg_sum<4>(nq, h, [&](int q, int k, double (&t)[4]) {
    const double x = X[xoff(q) + k];
    t[0] = B[q * h + k]; t[1] = x <= q05 ? 1.0 : 0.0; t[2] = x <= q95 ? 1.0 : 0.0; t[3] = x;
  }, cm, red);
  for (int e = tid; e < 4 * nq; e += DIAG_THREADS) cm[e / nq][e % nq] /= h;
  __syncthreads();
  // chain-mean variances (ddof 1) of the four series: every thread, same order
  double cmv[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    double mu = 0.0;
    for (int q = 0; q < nq; ++q) mu += cm[v][q];
    mu /= nq;
    double vb = 0.0;
    for (int q = 0; q < nq; ++q) { const double y = cm[v][q] - mu; vb = fma(y, y, vb); }
    cmv[v] = vb / (nq - 1);
  }
  // ---- mean and sd (ddof 1) of all C*S draws
  double mean_all, sd_all;
  {
    double s1[1] = {0.0};
    for (int e = tid; e < n; e += DIAG_THREADS) s1[0] += X[e];
    diag_block_sum<1>(s1, red);
    mean_all = s1[0] / n;
    double s2[1] = {0.0};
    for (int e = tid; e < n; e += DIAG_THREADS) { const double y = X[e] - mean_all; s2[0] = fma(y, y, s2[0]); }
    diag_block_sum<1>(s2, red);
    sd_all = sqrt(s2[0] / (n - 1));
  }
  // ---- autocovariances, two lags per pass, summed over the split chains
  DiagGeyer g[4];
  double rhat_b = 0.0;
  for (int t = -1;; t += 2) {                             // pass: lags t + 1, t + 2
    bool want[4];
    bool any = false;
#pragma unroll
    for (int v = 0; v < 4; ++v) { want[v] = t < 0 || (g[v].active && g[v].wants(t, h)); any |= want[v]; }
    if (!any) break;
    const int l1 = t + 1, l2 = t + 2, len = h - l1;
    double acc[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) acc[v] = 0.0;
    for (int e = tid; e < nq * len; e += DIAG_THREADS) {
      const int q = e / len, k = e - q * len;
      const double* zq = B + q * h;
      const double* xq = X + xoff(q);
      const bool two = k + l2 < h;
      const double x0 = xq[k], x1 = xq[k + l1], x2 = two ? xq[k + l2] : 0.0;
      double y0[4], y1[4], y2[4];
      y0[0] = zq[k] - cm[0][q]; y1[0] = zq[k + l1] - cm[0][q]; y2[0] = two ? zq[k + l2] - cm[0][q] : 0.0;
      y0[1] = (x0 <= q05 ? 1.0 : 0.0) - cm[1][q]; y1[1] = (x1 <= q05 ? 1.0 : 0.0) - cm[1][q];
      y2[1] = two ? (x2 <= q05 ? 1.0 : 0.0) - cm[1][q] : 0.0;
      y0[2] = (x0 <= q95 ? 1.0 : 0.0) - cm[2][q]; y1[2] = (x1 <= q95 ? 1.0 : 0.0) - cm[2][q];
      y2[2] = two ? (x2 <= q95 ? 1.0 : 0.0) - cm[2][q] : 0.0;
      y0[3] = x0 - cm[3][q]; y1[3] = x1 - cm[3][q]; y2[3] = two ? x2 - cm[3][q] : 0.0;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        acc[2 * v] = fma(y0[v], y1[v], acc[2 * v]);
        acc[2 * v + 1] = fma(y0[v], y2[v], acc[2 * v + 1]);
      }
    }
    diag_block_sum<8>(acc, red);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (!want[v]) continue;
      const double a1 = acc[2 * v] / h / nq, a2 = acc[2 * v + 1] / h / nq;     // dot / h, mean over the chains
      if (t < 0) {
        g[v].start(a1, a2, cmv[v], h);
        g[v].active = true;
        if (v == 0) {                                     // bulk R-hat: W = mean within-chain variance of z
          const double Bv = h * cmv[0], Wv = g[0].mean_var;
          rhat_b = sqrt((Bv / Wv + h - 1) / h);
        }
      } else {
        g[v].feed(a1, a2);
        if (!(g[v].even + g[v].odd > 0.0)) g[v].active = false;
      }
    }
  }
  if (tid == 0) {
    const double ess_b = g[0].ess(nq, h), e05 = g[1].ess(nq, h), e95 = g[2].ess(nq, h), ess_raw = g[3].ess(nq, h);
    a.out[0 * cells + oc] = rhat_f > rhat_b ? rhat_f : rhat_b;
    a.out[1 * cells + oc] = ess_b;
    a.out[2 * cells + oc] = e95 < e05 ? e95 : e05;
    a.out[3 * cells + oc] = sd_all / sqrt(ess_raw);
    a.out[4 * cells + oc] = mean_all;
  }
}

#define BTF_DIAG_SET(P)                                                                                  \
  P void diag_kernel<1>(DiagArgs); P void diag_kernel<2>(DiagArgs); P void diag_kernel<3>(DiagArgs);     \
  P void diag_kernel<4>(DiagArgs); P void diag_kernel<5>(DiagArgs); P void diag_kernel<6>(DiagArgs);     \
  P void diag_kernel<7>(DiagArgs); P void diag_kernel<8>(DiagArgs); P void diag_kernel<9>(DiagArgs);     \
  P void diag_kernel<10>(DiagArgs);

// instantiated in btf_diag.hip (its own compilation unit), declared here for the C-ABI unit
#ifndef BTF_DIAG_UNIT
#define BTF_X extern template __global__
BTF_DIAG_SET(BTF_X)
#undef BTF_X
#endif

}  // namespace btf
