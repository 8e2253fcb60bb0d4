// PSIS-LOO: Pareto-smoothed importance-sampling leave-one-curve-out  (BTF_K_CRITERIA)
//
// Vehtari, Gelman, Gabry (2017); Vehtari, Simpson, Gelman, Yao, Gabry (2024); the generalised Pareto fit of Zhang and
// Stephens (2009).  The written definition is functionalmf_amd/criteria.py: psis_curve / gpd_fit; this file implements
// the same steps on ll_s(i,j), the pointwise buffer [s][o] (o = i M + j) that crit_kernel (btf_criteria.h) leaves on the
// device.  Device scratch of a btf_crit_loo call: that buffer, 8 S N M bytes (1.05 GB at (512,256,64), S = 1000).
//
// loo_psis_kernel: one wave (one 64-lane workgroup) per curve, the whole curve in LDS:
//   LL[P] the log-likelihoods by sample, LR[P] the log ratios lr = min(ll) - ll sorted ascending with ties by ascending
//   sample index (bitonic on (lr, index) pairs, padded to the power of two P with +inf), IX[P] the sample of every sorted
//   position: 18 P bytes (18 KiB at S = 1000, 72 KiB at S = 4096).
//   cut = max(LR[S - Mt - 1], log DBL_MIN); the tail is the sorted positions with LR > cut (ties with the cut-off stay
//   outside), its excesses exp(lr) - exp(cut) overwrite LR there.  The Pareto fit puts grid point i of m = 30 +
//   floor(sqrt(n)) <= 58 on lane i (sum_j log1p(-b_i x_j) over the tail in ascending order, LDS broadcast reads); the
//   posterior weights, b, k and sigma come from fixed-order wave reductions; the smoothed tail overwrites the excesses.
//   Both log-sum-exps run over the sorted positions, lane-strided, with the same reductions.  No floating-point atomics:
//   two calls agree bit for bit.  Every branch around a barrier is wave-uniform (the workgroup is the wave, and what the
//   branches test comes out of a wave reduction or the kernel arguments).
//   Workgroup b takes curve (b % 8) * ceil(NM / 8) + b / 8: the workgroups that share an XCD's L2 read neighbouring
//   curves, whose samples share cache lines (the buffer is [s][o]; a curve is a stride-NM column of it).
//   Curves with a nan or +inf sample: all nan.  A -inf sample (an infinite ratio): elpd_loo = -inf, k = inf, weights nan.
//   No fit (Mt < 5, fewer than 5 tail samples, a smallest excess of 0, no surviving grid weight, a non-finite k or
//   sigma): k = inf, the unsmoothed estimate.
//   With WRITE_LW the normalised log weights overwrite the curve's column of the buffer.
//
// loo_mean_kernel: the leave-curve-out fitted curve, sum_s exp(lw_s(i,j)) f(w_i^s . v_jt^s) per cell, shaped like
//   crit_kernel: one workgroup per (column j, 64 rows), one lane per row, wave w takes the depth chunks w, w + LOO_WAVES,
//   ... of LOO_TC cells held in registers over all samples in ascending order (w_i^s: K per-lane loads; v_jt^s:
//   wave-uniform).  f: the transform codes of btf_posterior_summary (0 identity, 1 ilogit, 2 square).
#pragma once
#include "btf_device.h"
#include <math.h>

namespace btf {

constexpr int LOO_MAX_S = 4096;   // samples per call (the bound of btf_diag_eval): P <= 4096, 72 KiB of LDS
constexpr int LOO_MIN_TAIL = 5;   // fewer tail samples: no fit
constexpr int LOO_WAVES = 4;      // loo_mean_kernel: waves per workgroup
constexpr int LOO_TC = 16;        // loo_mean_kernel: depth cells per chunk

struct LooArgs {
  double* pw;            // [S][NM]: ll_s(o) in; with WRITE_LW the normalised log weights out
  const int* mt;         // [NM] tail lengths Mt, or null: mt_all for every curve
  int mt_all;
  int S, P, NM, per_xcd; // P: S rounded up to a power of two, >= 64; per_xcd = ceil(NM / 8)
  double* out;           // [2][NM]: elpd_loo, pareto_k
};

struct LooMeanArgs {
  const double* lw;      // [S][N][M] normalised log weights
  const double* W;       // [S][N][K]
  const double* V;       // [S][M][T][K]
  int S, N, M, T, transform;
  double* mean;          // (N,M,T)
};

__device__ __forceinline__ double loo_wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, WAVE));
  return v;
}
__device__ __forceinline__ double loo_wave_min(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, WAVE));
  return v;
}
__device__ __forceinline__ int loo_wave_sum_int(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

template <int WRITE_LW>
__global__ __launch_bounds__(WAVE) void loo_psis_kernel(LooArgs a) {
  extern __shared__ double loo_lds[];
  const int lane = threadIdx.x;
  const int S = a.S, P = a.P, NM = a.NM;
  const int o = (int)(blockIdx.x & 7) * a.per_xcd + (int)(blockIdx.x >> 3);
  if (o >= NM) return;                                     // (wave-uniform: the whole workgroup leaves)
  double* LL = loo_lds;
  double* LR = loo_lds + P;
  unsigned short* IX = reinterpret_cast<unsigned short*>(loo_lds + 2 * P);
  double* col = a.pw + o;
  const double NaN = __builtin_nan("");

  // ---- load the curve; classify
  double mn = INFINITY;
  int flags = 0;                                           // 1: a nan or +inf sample, 2: a -inf sample
  for (int s = lane; s < S; s += WAVE) {
    const double ll = col[(size_t)s * NM];
    LL[s] = ll;
    flags |= (ll != ll || ll == INFINITY) ? 1 : 0;
    flags |= (ll == -INFINITY) ? 2 : 0;
    mn = fmin(mn, ll);
  }
  flags = loo_wave_sum_int(flags & 1) > 0 ? 1 : (loo_wave_sum_int(flags & 2) > 0 ? 2 : 0);
  if (flags) {
    if (lane == 0) {
      a.out[o] = flags == 1 ? NaN : -INFINITY;
      a.out[NM + o] = flags == 1 ? NaN : INFINITY;
    }
    if (WRITE_LW)
      for (int s = lane; s < S; s += WAVE) col[(size_t)s * NM] = NaN;
    return;
  }
  mn = loo_wave_min(mn);
  __syncthreads();
  for (int e = lane; e < P; e += WAVE) {
    LR[e] = e < S ? mn - LL[e] : INFINITY;                 // lr = -ll - max(-ll), the same rounding
    IX[e] = (unsigned short)e;
  }
  __syncthreads();

  const int Mt = a.mt ? a.mt[o] : a.mt_all;
  int t0 = S, n = 0;                                       // the tail: sorted positions t0 .. S-1
  double cut = 0.0, ecut = 0.0, kfit = INFINITY, sigma = 0.0;
  bool fitted = false;
  if (Mt >= LOO_MIN_TAIL) {
    // ---- bitonic sort of (LR, IX), ascending, ties by ascending sample index (the pads, +inf with indices >= S, go last)
    const int half = P >> 1;
    for (int kk = 2; kk <= P; kk <<= 1) {
      for (int jj = kk >> 1; jj > 0; jj >>= 1) {
        for (int e = lane; e < half; e += WAVE) {
          const int i1 = ((e / jj) * 2 * jj) + (e % jj), i2 = i1 + jj;
          const double x1 = LR[i1], x2 = LR[i2];
          const unsigned short q1 = IX[i1], q2 = IX[i2];
          const bool up = (i1 & kk) == 0;
          const bool gt = x1 > x2 || (x1 == x2 && q1 > q2);
          if (gt == up) { LR[i1] = x2; LR[i2] = x1; IX[i1] = q2; IX[i2] = q1; }
        }
        __syncthreads();
      }
    }
    cut = fmax(LR[S - Mt - 1], -708.3964185322641);        // log(DBL_MIN)
    ecut = exp(cut);
    // the tail: LR > cut, strictly; the sorted order makes it the last n positions
    int above = 0;
    for (int e = S - Mt + lane; e < S; e += WAVE) above += LR[e] > cut ? 1 : 0;
    n = loo_wave_sum_int(above);
    t0 = S - n;
    __syncthreads();
    if (n >= LOO_MIN_TAIL) {
      double* X = LR + t0;
      for (int e = lane; e < n; e += WAVE) X[e] = exp(X[e]) - ecut;
      __syncthreads();
      if (X[0] > 0.0) {
        // ---- Zhang and Stephens: grid point i = lane + 1 of m
        const int m = 30 + (int)floor(sqrt((double)n));
        const double dn = (double)n;
        const double xq = X[(int)floor(dn / 4.0 + 0.5) - 1];
        const bool on = lane < m;
        const double bi = on ? 1.0 / X[n - 1] + (1.0 - sqrt((double)m / ((double)(lane + 1) - 0.5))) / (3.0 * xq) : 0.0;   // (idle lanes: log1p(0))
        double ks = 0.0;
        for (int e = 0; e < n; ++e) ks += log1p(-bi * X[e]);
        const double ki = ks / dn;
        const double li = dn * (log(-bi / ki) - ki - 1.0);
        double den = 0.0;
        for (int e = 0; e < m; ++e) den += exp(__shfl(li, e, WAVE) - li);
        double wi = 1.0 / den;
        wi = (on && wi >= 10.0 * 2.220446049250313e-16) ? wi : 0.0;      // (a nan weight is dropped too)
        const double wsum = wave_sum(wi);
        const double bp = wave_sum(on ? (wi / wsum) * bi : 0.0);
        double kp = 0.0;
        for (int e = lane; e < n; e += WAVE) kp += log1p(-bp * X[e]);
        kp = wave_sum(kp) / dn;
        sigma = -kp / bp;
        const double kadj = (dn * kp + 5.0) / (dn + 10.0);
        if (isfinite(kadj) && isfinite(sigma)) { fitted = true; kfit = kadj; }   // (no surviving weight: bp, kadj nan)
      }
      __syncthreads();
      // ---- the smoothed tail in ascending order, or the raw log ratios back
      for (int e = lane; e < n; e += WAVE) {
        double v;
        if (fitted) {
          const double l1p = log1p(-((double)(e + 1) - 0.5) / (double)n);
          const double q = kfit == 0.0 ? -sigma * l1p : sigma * expm1(-kfit * l1p) / kfit;
          v = log(q + ecut);
        } else {
          v = mn - LL[IX[t0 + e]];
        }
        X[e] = v;
      }
      __syncthreads();
    }
  }

  // ---- truncate at 0, normalise, elpd_loo = logsumexp(lw + ll)   (sorted positions; unsorted when Mt < 5)
  double m1 = -INFINITY;
  for (int e = lane; e < S; e += WAVE) {
    const double v = fmin(LR[e], 0.0);                     // (fmin drops a nan: as the definition's np.minimum does not)
    LR[e] = LR[e] != LR[e] ? LR[e] : v;
    m1 = fmax(m1, LR[e]);
  }
  __syncthreads();
  m1 = loo_wave_max(m1);
  double s1 = 0.0;
  for (int e = lane; e < S; e += WAVE) s1 += exp(LR[e] - m1);
  const double lse = m1 + log(wave_sum(s1));
  double m2 = -INFINITY;
  for (int e = lane; e < S; e += WAVE) {
    const double lw = LR[e] - lse;
    const int s = IX[e];
    if (WRITE_LW) col[(size_t)s * NM] = lw;
    const double v = lw + LL[s];
    LR[e] = v;                                             // (each lane rereads only its own positions)
    m2 = fmax(m2, v);
  }
  m2 = loo_wave_max(m2);
  double s2 = 0.0;
  for (int e = lane; e < S; e += WAVE) s2 += exp(LR[e] - m2);
  s2 = wave_sum(s2);
  if (lane == 0) {
    a.out[o] = m2 + log(s2);
    a.out[NM + o] = kfit;
  }
}

template <int K>
__global__ __launch_bounds__(LOO_WAVES * WAVE) void loo_mean_kernel(LooMeanArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int j = blockIdx.y;
  const int i = blockIdx.x * WAVE + lane;
  const bool row_ok = i < a.N;
  const int ic = row_ok ? i : a.N - 1;                     // clamped row for the loads of the lanes past the end
  const int N = a.N, M = a.M, T = a.T;
  const int nch = (T + LOO_TC - 1) / LOO_TC;
  for (int ch = wv; ch < nch; ch += LOO_WAVES) {
    const int t0 = ch * LOO_TC, tn = min(LOO_TC, T - t0);
    double acc[LOO_TC];
#pragma unroll
    for (int u = 0; u < LOO_TC; ++u) acc[u] = 0.0;
    for (int s = 0; s < a.S; ++s) {
      const double* __restrict__ wp = a.W + ((size_t)s * N + ic) * K;
      const double* __restrict__ vp = a.V + (((size_t)s * M + j) * T + t0) * K;
      const double wt = exp(a.lw[((size_t)s * N + ic) * M + j]);
      double w[K];
#pragma unroll
      for (int k = 0; k < K; ++k) w[k] = wp[k];
#pragma unroll
      for (int u = 0; u < LOO_TC; ++u) {
        if (u < tn) {
          double eta = 0.0;
#pragma unroll
          for (int k = 0; k < K; ++k) eta = fma(w[k], vp[u * K + k], eta);
          const double f = a.transform == 1 ? 1.0 / (1.0 + exp(-eta)) : (a.transform == 2 ? eta * eta : eta);
          acc[u] = fma(wt, f, acc[u]);
        }
      }
    }
    if (row_ok) {
#pragma unroll
      for (int u = 0; u < LOO_TC; ++u)
        if (u < tn) a.mean[((size_t)i * M + j) * T + t0 + u] = acc[u];
    }
  }
}

#define BTF_LOO_SET(P)                                                                                   \
  P void loo_psis_kernel<0>(LooArgs); P void loo_psis_kernel<1>(LooArgs);                                \
  P void loo_mean_kernel<1>(LooMeanArgs); P void loo_mean_kernel<2>(LooMeanArgs); P void loo_mean_kernel<3>(LooMeanArgs); \
  P void loo_mean_kernel<4>(LooMeanArgs); P void loo_mean_kernel<5>(LooMeanArgs); P void loo_mean_kernel<6>(LooMeanArgs); \
  P void loo_mean_kernel<7>(LooMeanArgs); P void loo_mean_kernel<8>(LooMeanArgs); P void loo_mean_kernel<9>(LooMeanArgs); \
  P void loo_mean_kernel<10>(LooMeanArgs);

// instantiated in btf_loo.hip (its own compilation unit), declared here for the C-ABI unit
#ifndef BTF_LOO_UNIT
#define BTF_X extern template __global__
BTF_LOO_SET(BTF_X)
#undef BTF_X
#endif

}  // namespace btf
