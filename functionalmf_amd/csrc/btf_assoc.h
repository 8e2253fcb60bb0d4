// Posterior feature association: the regression of a curve functional on a row feature's probability, per kept sample
// (counted under BTF_K_CRITERIA)
//
// Reference: doseresponse/feature_importance.py:39-54 regresses, for every (feature, drug) pair, the per-row AUC of the
// posterior-mean curves on the posterior-mean feature probability w_i . u_f (scipy.stats.linregress) - on posterior means
// only.  Here, for kept sample s, feature f and column j, with y_i = one functional of btf_functionals.h of the curve
// (i,j), x_i = w_i^s . u_f^s and I = {i : y_i defined} (an undefined crossing leaves the row out), n = |I|:
//   Sxx, Syy, Sxy centred sums over I;  r = Sxy / sqrt(Sxx Syy);  slope = Sxy / Sxx;  defined iff n >= 3, Sxx > 0, Syy > 0
// (functionalmf_amd/association.py restates this in numpy; that module is the definition).  x is linear in w, so every
// moment of x over the rows is a K-dimensional form in moments of W that do not depend on the feature:
//   xbar = u . wbar,   Sxy = u . c,   Sxx = u' C u,     c = sum_I (w - wbar)(y - ybar),   C = sum_I (w - wbar)(w - wbar)'
// and the S x F x M x N product is never formed: the data-sized work is one more pass over the functional values.
//
// Staged through a scratch buffer in chunks of SAMPLES, vals[column][sample of the chunk][row], written by the unchanged
// func_sweep_kernel (one functional, all M columns: the values of posterior_functionals(pointwise=True) bit for bit).
//   assoc_moments_kernel<K>  one wave per (column, sample of the chunk), lanes along rows.  Pass 1: n, ybar, wbar.  Pass 2:
//       the CENTRED Syy, c (K) and C (K(K+1)/2) - not raw sums minus a product of means.  Every lane owns the rows
//       lane, lane + 64, ... whatever the chunk, and the 64 partial sums are added by the xor butterfly of wave_sum (both
//       partners form the same commutative sum): a fixed order.  3 + 2K + K(K+1)/2 doubles per (sample, column), kept for
//       all S samples:  [n, ybar, Syy, wbar (K), c (K), C (packed lower triangle)].
//   assoc_reduce_kernel<K>   one workgroup per tile of `cells` consecutive FEATURES of one column: the tile shares the
//       (sample, column) moments, the larger item (28 doubles at K = 5 against the 5 of u_f^s), so a pair re-reads
//       K + (3 + 2K + K(K+1)/2) / cells doubles per sample (8.5 at K = 5, cells = 8, against 33 with one pair per
//       workgroup).  Thread -> (pair of the tile, sample): r and slope from u_f^s and the moments go to an LDS row per (pair,
//       requested statistic), padded to the power of two P >= S with +inf, which also stands for an undefined sample ("nan
//       last"); a bitonic network sorts the rows; mean, M2 (two passes), the counts and the percentiles (numpy's linear rule
//       over the defined samples) follow over the sorted row in FUNC_PARTS interleaved partial sums added in part order.
//       cells = min(16 rows, 64 KiB / (8 P)) / statistics: S = 1000, one statistic: 8 pairs, 64 KiB of LDS.
//       The workgroups of the first feature tile also sum n over the samples (integers in doubles: exact in any order).
//   assoc_values_kernel<K>   the raw per-sample statistics of the requested (feature, column) pairs, nan where undefined:
//       the same assoc_stat as the reduce kernel on the same moments.
// The plug-in table of the reference ("of_means"):
//   assoc_pbar_kernel<K>     Pbar' [F][N] = mean_s W_s U_s', one thread per (row, 8 features), samples in order.
//   assoc_gbar_kernel        per chunk, one thread per curve: the running sum and count of the defined values, samples in
//       order (the running sum is reloaded, so the chunking cannot change a bit); assoc_gbar_finish_kernel divides (nan
//       where no sample is defined: that row is left out of the column's regression).
//   assoc_cross_kernel       one wave per (feature, column): two passes over the N rows of Pbar' and gbar' (both with rows
//       contiguous), centred sums, then r, slope, intercept, stderr, n; the first column's waves add sd_x over all rows.
// Build (hipcc -O3, gfx950; -Rpass-analysis=kernel-resource-usage): no kernel of this unit uses scratch or spills.
//   assoc_moments_kernel  K = 5: 102 VGPRs (4 waves per SIMD); K = 10: 256 VGPRs, one 64-thread wave per SIMD (55 Gram + 10
//                         + 1 accumulators, e and wbar in registers); no LDS
//   assoc_reduce_kernel   K = 5: 64 VGPRs; K = 10: 68 VGPRs; LDS: 64 KiB of rows + 6.2 KiB static, two workgroups per CU
//                         (S > 4096 with both statistics: two rows of 64 KiB, one workgroup per CU)
//   assoc_pbar_kernel     K = 5: 44 VGPRs;  assoc_cross_kernel 40 VGPRs;  assoc_values_kernel K = 5: 64 VGPRs
// fp64 throughout, no floating-point atomics, every sum in a fixed order.
#pragma once
#include "btf_device.h"
#include "btf_functionals.h"

namespace btf {

enum { ASSOC_R = 0, ASSOC_SLOPE = 1, ASSOC_NSTATS = 2 };
constexpr int ASSOC_THREADS = 256;
constexpr int ASSOC_SORT_LDS = 64 * 1024;     // bytes of LDS for the rows of one reduce workgroup
constexpr int ASSOC_ROWS = 16;                // at most this many (pair, statistic) rows per reduce workgroup
constexpr int ASSOC_FT = 8;                   // features per thread of assoc_pbar_kernel
constexpr int ASSOC_OM = 5;                   // planes of the of_means table: r, slope, intercept, stderr, n

__host__ __device__ constexpr int assoc_nmom(int K) { return 3 + 2 * K + K * (K + 1) / 2; }

struct AssocArgs {
  const double* vals;            // [M][sc][N]: this chunk's values
  const double* W;               // [S][N][K]
  const double* U;               // [S][F][K]
  int S, N, M, F;
  int s0, sc;                    // this chunk: samples s0 .. s0 + sc - 1
  double* mom;                   // [S][M][assoc_nmom(K)]
  // reduce
  int nst, st[ASSOC_NSTATS];     // requested statistics, in output order
  int P, pshift, cells;          // padded row length (1 << pshift >= max(S, 2)), pairs per reduce workgroup
  const double* q; int nq;
  double* mean; double* var; double* prob;   // [nst][F][M]
  double* quant;                 // [nst][nq][F][M]
  double* defined;               // [F][M]
  double* nmean;                 // [M]
  int npairs; const int* pairs;  // (f, j) rows
  double* values;                // [nst][npairs][S]
  // of_means
  double* pbar;                  // [F][N]
  double* gbar;                  // [M][N]: running sums, then the means
  int* gcnt;                     // [M][N]
  double* om;                    // [ASSOC_OM][F][M]
  double* sdx; double* sdy;      // (F,), (M,)
};

using AssocKernel = void (*)(AssocArgs);
AssocKernel assoc_moments_fn(int K);          // null outside K = 1..10
AssocKernel assoc_reduce_fn(int K);
AssocKernel assoc_values_fn(int K);
AssocKernel assoc_pbar_fn(int K);
AssocKernel assoc_gbar_fn();
AssocKernel assoc_gbar_finish_fn();
AssocKernel assoc_cross_fn();

#ifdef BTF_ASSOC_UNIT
template <int K>
__global__ __launch_bounds__(WAVE) void assoc_moments_kernel(AssocArgs a) {
  const int lane = threadIdx.x, j = blockIdx.x, sl = blockIdx.y, N = a.N;
  const double* __restrict__ y = a.vals + ((size_t)j * a.sc + sl) * N;
  const double* __restrict__ W = a.W + (size_t)(a.s0 + sl) * N * K;
  // ---- pass 1: n, ybar, wbar over the defined rows
  double cnt = 0.0, sy = 0.0, wb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) wb[k] = 0.0;
  for (int i = lane; i < N; i += WAVE) {
    const double v = y[i];
    const bool ok = v == v;
    cnt += ok ? 1.0 : 0.0;
    sy += ok ? v : 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) { const double w = W[(size_t)i * K + k]; wb[k] += ok ? w : 0.0; }
  }
  cnt = wave_sum(cnt);
  const double ybar = cnt > 0.0 ? wave_sum(sy) / cnt : 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) { const double t = wave_sum(wb[k]); wb[k] = cnt > 0.0 ? t / cnt : 0.0; }
  // ---- pass 2: the centred sums
  double syy = 0.0, c[K], G[tri(K)];
#pragma unroll
  for (int k = 0; k < K; ++k) c[k] = 0.0;
#pragma unroll
  for (int t = 0; t < tri(K); ++t) G[t] = 0.0;
  for (int i = lane; i < N; i += WAVE) {
    const double v = y[i];
    const bool ok = v == v;
    const double d = ok ? v - ybar : 0.0;
    double e[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { const double w = W[(size_t)i * K + k]; e[k] = ok ? w - wb[k] : 0.0; }
    syy = fma(d, d, syy);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      c[k] = fma(e[k], d, c[k]);
#pragma unroll
      for (int l = 0; l <= k; ++l) G[lidx(k, l)] = fma(e[k], e[l], G[lidx(k, l)]);
    }
  }
  syy = wave_sum(syy);
#pragma unroll
  for (int k = 0; k < K; ++k) c[k] = wave_sum(c[k]);
#pragma unroll
  for (int t = 0; t < tri(K); ++t) G[t] = wave_sum(G[t]);
  if (lane == 0) {
    double* __restrict__ o = a.mom + ((size_t)(a.s0 + sl) * a.M + j) * assoc_nmom(K);
    o[0] = cnt; o[1] = ybar; o[2] = syy;
#pragma unroll
    for (int k = 0; k < K; ++k) { o[3 + k] = wb[k]; o[3 + K + k] = c[k]; }
#pragma unroll
    for (int t = 0; t < tri(K); ++t) o[3 + 2 * K + t] = G[t];
  }
}

// r and slope of one (sample, feature, column) from u = u_f^s and the (s, j) moments; false: undefined
template <int K>
__device__ __forceinline__ bool assoc_stat(const double* __restrict__ m, const double* __restrict__ up, double& r, double& slope) {
  double u[K];
#pragma unroll
  for (int k = 0; k < K; ++k) u[k] = up[k];
  const double n = m[0], syy = m[2];
  double sxy = 0.0, sxx = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) sxy = fma(u[k], m[3 + K + k], sxy);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double t = 0.0;                                           // (C u)_k from the packed lower triangle
#pragma unroll
    for (int l = 0; l < K; ++l) t = fma(m[3 + 2 * K + (l <= k ? lidx(k, l) : lidx(l, k))], u[l], t);
    sxx = fma(u[k], t, sxx);
  }
  const bool ok = n >= 3.0 && sxx > 0.0 && syy > 0.0;
  r = ok ? sxy / sqrt(sxx * syy) : __builtin_nan("");
  slope = ok ? sxy / sxx : __builtin_nan("");
  return ok;
}

template <int K>
__global__ __launch_bounds__(ASSOC_THREADS) void assoc_reduce_kernel(AssocArgs a) {
  extern __shared__ double srt[];                 // [cells][nst][P]
  __shared__ double psum[ASSOC_ROWS][FUNC_PARTS];
  __shared__ int pcnt[ASSOC_ROWS][FUNC_PARTS], ppos[ASSOC_ROWS][FUNC_PARTS];
  __shared__ double rmean[ASSOC_ROWS];
  __shared__ int rcnt[ASSOC_ROWS];
  __shared__ double nred[ASSOC_THREADS];
  constexpr int NMOM = assoc_nmom(K);
  const int cells = a.cells, nst = a.nst, P = a.P, S = a.S, M = a.M, F = a.F;
  const int j = blockIdx.x % M, f0 = (blockIdx.x / M) * cells;
  const int nc = min(cells, F - f0), rows = cells * nst, nrows = nc * nst;
  const int tid = threadIdx.x;
  const double inf = __builtin_inf();
  // ---- values: thread -> (pair c of the tile, sample s); the `cells` pairs of a sample share its moments
  for (int e = tid; e < cells * P; e += ASSOC_THREADS) {
    const int c = e % cells, s = e / cells;
    double r = inf, slope = inf;
    if (s < S && c < nc) {
      double rr, sl;
      if (assoc_stat<K>(a.mom + ((size_t)s * M + j) * NMOM, a.U + ((size_t)s * F + f0 + c) * K, rr, sl)) { r = rr; slope = sl; }
    }
    for (int t = 0; t < nst; ++t) srt[((size_t)c * nst + t) * P + s] = a.st[t] == ASSOC_R ? r : slope;
  }
  __syncthreads();
  // ---- bitonic sort of every row (ascending): undefined samples and padding (+inf) last
  const int half = P >> 1, hshift = a.pshift - 1;
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int e = tid; e < rows * half; e += ASSOC_THREADS) {
        const int rw = e >> hshift, p = e & (half - 1);
        const int i1 = ((p & ~(jj - 1)) << 1) | (p & (jj - 1)), i2 = i1 + jj;
        double* row = srt + (size_t)rw * P;
        const double va = row[i1], vb = row[i2];
        const bool up = (i1 & kk) == 0;
        if ((va > vb) == up) { row[i1] = vb; row[i2] = va; }
      }
      __syncthreads();
    }
  }
  // ---- pass 1: sum, count of the defined samples and of the positive ones; part p takes s = p, p + PARTS, ...
  for (int e = tid; e < nrows * FUNC_PARTS; e += ASSOC_THREADS) {
    const int rw = e / FUNC_PARTS, p = e % FUNC_PARTS;
    const double* row = srt + (size_t)rw * P;
    double sum = 0.0;
    int cnt = 0, pos = 0;
    for (int s = p; s < S; s += FUNC_PARTS) {
      const double v = row[s];
      if (v < inf) { sum += v; ++cnt; pos += v > 0.0 ? 1 : 0; }
    }
    psum[rw][p] = sum; pcnt[rw][p] = cnt; ppos[rw][p] = pos;
  }
  __syncthreads();
  for (int rw = tid; rw < nrows; rw += ASSOC_THREADS) {
    double sum = 0.0;
    int cnt = 0, pos = 0;
    for (int p = 0; p < FUNC_PARTS; ++p) { sum += psum[rw][p]; cnt += pcnt[rw][p]; pos += ppos[rw][p]; }
    const int c = rw / nst, t = rw - c * nst;
    const size_t o = ((size_t)t * F + f0 + c) * M + j;
    const double mean = cnt > 0 ? sum / cnt : __builtin_nan("");
    rmean[rw] = mean; rcnt[rw] = cnt;
    a.mean[o] = mean;
    a.prob[o] = cnt > 0 ? (double)pos / cnt : __builtin_nan("");
    if (t == 0) a.defined[(size_t)(f0 + c) * M + j] = (double)cnt / S;
  }
  __syncthreads();
  // ---- pass 2: squared deviations from the mean, same parts and order
  for (int e = tid; e < nrows * FUNC_PARTS; e += ASSOC_THREADS) {
    const int rw = e / FUNC_PARTS, p = e % FUNC_PARTS;
    const double* row = srt + (size_t)rw * P;
    const double mean = rmean[rw];
    double sum = 0.0;
    for (int s = p; s < S; s += FUNC_PARTS) {
      const double v = row[s];
      if (v < inf) { const double d = v - mean; sum = fma(d, d, sum); }
    }
    psum[rw][p] = sum;
  }
  __syncthreads();
  for (int rw = tid; rw < nrows; rw += ASSOC_THREADS) {
    double sum = 0.0;
    for (int p = 0; p < FUNC_PARTS; ++p) sum += psum[rw][p];
    const int c = rw / nst, t = rw - c * nst, cnt = rcnt[rw];
    a.var[((size_t)t * F + f0 + c) * M + j] = cnt > 1 ? sum / (cnt - 1) : cnt == 1 ? 0.0 : __builtin_nan("");
  }
  // ---- percentiles over the defined samples: numpy's default ('linear')
  for (int e = tid; e < nrows * a.nq; e += ASSOC_THREADS) {
    const int rw = e % nrows, qi = e / nrows;
    const int c = rw / nst, t = rw - c * nst, cnt = rcnt[rw];
    const double* row = srt + (size_t)rw * P;
    double v = __builtin_nan("");
    if (cnt > 0) {
      const double pos = a.q[qi] * 0.01 * (cnt - 1);
      int lo = (int)floor(pos);
      lo = max(0, min(lo, cnt - 1));
      const int hi = min(lo + 1, cnt - 1);
      const double vl = row[lo], vh = row[hi];
      v = vl + (pos - lo) * (vh - vl);
    }
    a.quant[(((size_t)t * a.nq + qi) * F + f0 + c) * M + j] = v;
  }
  // ---- the first feature tile: n of the column summed over the samples (integers: exact, whatever the order)
  if (f0 == 0) {
    double sum = 0.0;
    for (int s = tid; s < S; s += ASSOC_THREADS) sum += a.mom[((size_t)s * M + j) * NMOM];
    nred[tid] = sum;
    __syncthreads();
    for (int w = ASSOC_THREADS / 2; w > 0; w >>= 1) {
      if (tid < w) nred[tid] += nred[tid + w];
      __syncthreads();
    }
    if (tid == 0) a.nmean[j] = nred[0] / S;
  }
}

template <int K>
__global__ __launch_bounds__(ASSOC_THREADS) void assoc_values_kernel(AssocArgs a) {
  const int p = blockIdx.x, f = a.pairs[2 * p], j = a.pairs[2 * p + 1];
  for (int s = threadIdx.x; s < a.S; s += ASSOC_THREADS) {
    double r, slope;
    assoc_stat<K>(a.mom + ((size_t)s * a.M + j) * assoc_nmom(K), a.U + ((size_t)s * a.F + f) * K, r, slope);
    for (int t = 0; t < a.nst; ++t) a.values[((size_t)t * a.npairs + p) * a.S + s] = a.st[t] == ASSOC_R ? r : slope;
  }
}

// Pbar' [f][i] = (1 / S) sum_s w_i^s . u_f^s, samples in order; lanes along rows, ASSOC_FT features per thread (their
// u_f^s at wave-uniform addresses)
template <int K>
__global__ __launch_bounds__(ASSOC_THREADS) void assoc_pbar_kernel(AssocArgs a) {
  const int N = a.N, F = a.F, S = a.S;
  const int rb = (N + ASSOC_THREADS - 1) / ASSOC_THREADS;
  const int i = (blockIdx.x % rb) * ASSOC_THREADS + threadIdx.x, f0 = (blockIdx.x / rb) * ASSOC_FT;
  const int ic = min(i, N - 1);
  double acc[ASSOC_FT];
#pragma unroll
  for (int g = 0; g < ASSOC_FT; ++g) acc[g] = 0.0;
  for (int s = 0; s < S; ++s) {
    const double* __restrict__ wp = a.W + ((size_t)s * N + ic) * K;
    double w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = wp[k];
#pragma unroll
    for (int g = 0; g < ASSOC_FT; ++g) {
      const double* __restrict__ up = a.U + ((size_t)s * F + min(f0 + g, F - 1)) * K;
      double d = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) d = fma(w[k], up[k], d);
      acc[g] += d;
    }
  }
  if (i < N) {
#pragma unroll
    for (int g = 0; g < ASSOC_FT; ++g)
      if (f0 + g < F) a.pbar[(size_t)(f0 + g) * N + i] = acc[g] / S;
  }
}

// the running sum and count of the defined values of every curve over this chunk's samples, in sample order
__global__ __launch_bounds__(ASSOC_THREADS) void assoc_gbar_kernel(AssocArgs a) {
  const int N = a.N, rb = (N + ASSOC_THREADS - 1) / ASSOC_THREADS;
  const int i = (blockIdx.x % rb) * ASSOC_THREADS + threadIdx.x, j = blockIdx.x / rb;
  if (i >= N) return;
  const size_t o = (size_t)j * N + i;
  double sum = a.gbar[o];
  int cnt = a.gcnt[o];
  const double* __restrict__ y = a.vals + (size_t)j * a.sc * N + i;
  for (int s = 0; s < a.sc; ++s) {
    const double v = y[(size_t)s * N];
    if (v == v) { sum += v; ++cnt; }
  }
  a.gbar[o] = sum; a.gcnt[o] = cnt;
}

__global__ __launch_bounds__(ASSOC_THREADS) void assoc_gbar_finish_kernel(AssocArgs a) {
  const size_t o = (size_t)blockIdx.x * ASSOC_THREADS + threadIdx.x;
  if (o < (size_t)a.N * a.M) { const int cnt = a.gcnt[o]; a.gbar[o] = cnt > 0 ? a.gbar[o] / cnt : __builtin_nan(""); }
}

// one wave per (feature, column): the regression of gbar[:, j] on Pbar[:, f] over the rows with a defined gbar
__global__ __launch_bounds__(ASSOC_THREADS) void assoc_cross_kernel(AssocArgs a) {
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const int N = a.N, M = a.M, F = a.F, cb = (M + 3) / 4;
  const int j = (blockIdx.x % cb) * 4 + wv, f = blockIdx.x / cb;
  if (j >= M) return;                               // (no barrier below)
  const double* __restrict__ x = a.pbar + (size_t)f * N;
  const double* __restrict__ y = a.gbar + (size_t)j * N;
  double cnt = 0.0, sx = 0.0, sy = 0.0, sxa = 0.0;
  for (int i = lane; i < N; i += WAVE) {
    const double xv = x[i], yv = y[i];
    const bool ok = yv == yv;
    cnt += ok ? 1.0 : 0.0; sx += ok ? xv : 0.0; sy += ok ? yv : 0.0; sxa += xv;
  }
  cnt = wave_sum(cnt);
  const double xbar = cnt > 0.0 ? wave_sum(sx) / cnt : 0.0, ybar = cnt > 0.0 ? wave_sum(sy) / cnt : 0.0;
  const double xall = wave_sum(sxa) / N;
  double sxx = 0.0, syy = 0.0, sxy = 0.0, sxxa = 0.0;
  for (int i = lane; i < N; i += WAVE) {
    const double xv = x[i], yv = y[i];
    const bool ok = yv == yv;
    const double dx = ok ? xv - xbar : 0.0, dy = ok ? yv - ybar : 0.0, da = xv - xall;
    sxx = fma(dx, dx, sxx); syy = fma(dy, dy, syy); sxy = fma(dx, dy, sxy); sxxa = fma(da, da, sxxa);
  }
  sxx = wave_sum(sxx); syy = wave_sum(syy); sxy = wave_sum(sxy); sxxa = wave_sum(sxxa);
  if (lane == 0) {
    const bool ok = cnt >= 3.0 && sxx > 0.0 && syy > 0.0;
    const double nan = __builtin_nan("");
    const double r = ok ? sxy / sqrt(sxx * syy) : nan, slope = ok ? sxy / sxx : nan;
    const size_t o = (size_t)f * M + j, FM = (size_t)F * M;
    a.om[o] = r;
    a.om[FM + o] = slope;
    a.om[2 * FM + o] = ok ? ybar - slope * xbar : nan;
    a.om[3 * FM + o] = ok ? sqrt(fmax(1.0 - r * r, 0.0) * syy / sxx / (cnt - 2.0)) : nan;
    a.om[4 * FM + o] = cnt;
    if (f == 0) a.sdy[j] = cnt > 0.0 ? sqrt(syy / cnt) : nan;
    if (j == 0) a.sdx[f] = sqrt(sxxa / N);
  }
}
#endif  // BTF_ASSOC_UNIT

}  // namespace btf
