// Folding new rows into a fitted posterior  (counted under BTF_K_CRITERIA)
//
// Reference: given V the rows of W are conditionally independent (factor.py:333), and the prior of a row is N(0, sigma2 I).
// For a NEW row with observations y (any missing pattern) and kept sample s, what _resample_W (factor.py:333-362) does
// for a row of the fitted tensor holds for the new one:
//     Q_s = sum_{(j,t)} c_jt v_jt^s v_jt^s' / nu2_s + I / sigma2_s      b_s = sum_{(j,t)} ysum_jt v_jt^s / nu2_s
//     w_new^s = Q_s^-1 b_s + L^-T z,   Q_s = L L'                        (factor.py:357-362)
// (c_jt observed replicates of the cell, ysum_jt their sum), one draw per kept sample.  Binomial rows (factor.py:437-460)
// run a short chain per (sample, row) from w = 0: omega_jt ~ PG(n_jt, w . v_jt) by the exact sampler of btf_pg_exact.h,
// then the same draw with the weights omega_jt in the place of c_jt / nu2 and kappa_jt = y_jt - n_jt / 2 in the place of
// ysum_jt / nu2.  functionalmf_amd/fold_in.py restates the Gaussian conditional in numpy; that module is the definition.
//
// ONE launch, fold_in_kernel<K, FAMILY>: a workgroup of FOLD_PARTS waves owns (sample s, 64 new rows) - for the whole
// inner chain in the Binomial family - with one lane per row.
//   accumulation   wave p takes the cells jt = p, p + FOLD_PARTS, ... in ascending order.  v_jt^s is read at a
//       wave-uniform address (scalar loads: every V tile is read once for the 64 rows of the workgroup), the statistics of
//       the cell are one coalesced load over the rows ([cell][row] layout), and each lane keeps the K(K+1)/2 + K running
//       sums of its row in registers: t_a = c v_a once per (cell, row), then K(K+1)/2 + K fused multiply-adds on the VALU.
//       A missing cell has c = ysum = 0 and adds exact zeros: complete and incomplete rows take the same path, same bits.
//   reduction      the FOLD_PARTS partial sums of a row are added in part order through LDS: ((p0 + p1) + p2) + p3.
//       FOLD_PARTS is part of the result's definition, not of the launch geometry: a sum never depends on the grid, on
//       how many rows or samples a call holds, or on where the states come from.  No atomics on floating-point data.
//   solve and draw wave 0, lane = row: packed K x K Cholesky in registers, mean by two triangular solves, L^-T z with z the
//       caller's normals or Philox keyed (seed, stream = global sample index << 32 | row, index = sweep K + k) - never a
//       thread or block index.  A non-positive pivot raises the status flag and leaves the smallest failing
//       (sample, row) pair (integer atomicMin): BTF_ENOTPD with btf_fail_index = sample * nrows_new + row.
//   Binomial       w of the rows goes back to all waves through LDS and the next round starts; the Polya-Gamma stream
//       of a cell is keyed by (a Philox word of (seed, sample, row), sweep * MT + jt).
// Scratch: none beyond the inputs and outputs - the row statistics 2 R MT doubles, W and W_mean 2 S R K doubles, and the
// summary's (1 + nq) R MT doubles.  The summary stage is posterior_summary_kernel itself on the device-resident W and V.
// fp64 throughout (the accepted Polya-Gamma variate is the f32 candidate of btf_pg_exact.h, as in the sampler's sweeps).
#pragma once
#include "btf_device.h"
#include <math.h>

namespace btf {

enum { FOLD_GAUSSIAN = 0, FOLD_BINOMIAL = 1 };
constexpr int FOLD_PARTS = 4;                  // waves per workgroup = interleaved partial sums per row (fixed: part of the definition)
constexpr int FOLD_MAX_TRIALS = 32;            // PG_AUTO_EXACT_MAX: the counts pg_exact=None draws exactly

struct FoldArgs {
  const double* V;          // [S][MT][K]
  const double* noise;      // nu2 of sample s at noise[s * nstride] (Gaussian); null: 1
  const double* sigma2;     // sigma2 of sample s at sigma2[s * sstride]
  const double* cnt;        // [MT][R]  Gaussian: observed replicates; Binomial: trials of the observed cells (0: missing)
  const double* ysum;       // [MT][R]  Gaussian: sum of the observed replicates; Binomial: kappa = successes - trials / 2
  const double* z;          // [S][R][K] standard normals, or null: the device generator
  double* W;                // [S][R][K]
  double* Wmean;            // [S][R][K] or null
  int* status;              // [0]: 1 after a non-positive pivot, [1]: the smallest failing sample * R + row
  unsigned long long seed;
  long long sample0;        // global index of sample 0 of this call (generator keys)
  int nstride, sstride;
  int S, R, MT, sweeps;
};

// the kernels live in btf_fold_in.hip (a compilation unit of their own); the C-ABI unit launches them through this
using FoldKernel = void (*)(FoldArgs);
FoldKernel fold_in_fn(int K, int family);      // null outside K = 1..10, family = 0..1

}  // namespace btf

#ifdef BTF_FOLD_UNIT
#include "btf_pg_exact.h"

namespace btf {

template <int K, int FAM>
__global__ __launch_bounds__(FOLD_PARTS * WAVE) void fold_in_kernel(FoldArgs a) {
  constexpr int KK = tri(K), NA = KK + K, NT = FOLD_PARTS * WAVE;
  __shared__ double red[NA][WAVE];
  __shared__ double wsh[K][WAVE];
  __shared__ uint4 rec_g[FAM == FOLD_BINOMIAL ? NT : 1], rec_p[FAM == FOLD_BINOMIAL ? NT : 1];
  __shared__ float pg_out[FAM == FOLD_BINOMIAL ? NT : 1];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int s = blockIdx.x, R = a.R, MT = a.MT;
  const int r = blockIdx.y * WAVE + lane;
  const bool row_ok = r < R;
  const int rc = row_ok ? r : R - 1;                         // clamped row for the loads of the lanes past the end
  const double* __restrict__ V = a.V + (size_t)s * MT * K;
  const double* __restrict__ cnt = a.cnt + rc;
  const double* __restrict__ ysum = a.ysum + rc;
  const unsigned long long sg = (unsigned long long)(a.sample0 + s);
  const unsigned long long stream = (sg << 32) | (unsigned long long)(unsigned)r;
  unsigned long long pg_key = 0;
  if constexpr (FAM == FOLD_BINOMIAL) {
    uint32_t kw[4];
    Philox::gen(a.seed, stream, 0x666f6c64ULL << 24, kw);    // a counter the normals of the stream never reach
    pg_key = ((unsigned long long)kw[1] << 32) | kw[0];
  }
  double w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = 0.0;
  const int nsweeps = FAM == FOLD_BINOMIAL ? a.sweeps : 1;
  for (int sw = 0; sw < nsweeps; ++sw) {
    double acc[NA];
#pragma unroll
    for (int e = 0; e < NA; ++e) acc[e] = 0.0;
    // ---- accumulation: this wave's cells, ascending
#pragma unroll 2
    for (int jt = wv; jt < MT; jt += FOLD_PARTS) {
      double v[K];
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = V[(size_t)jt * K + k];
      const double y = ysum[(size_t)jt * R];
      double wt = cnt[(size_t)jt * R];
      if constexpr (FAM == FOLD_BINOMIAL) {
        double psi = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) psi = fma(w[k], v[k], psi);
        const int nb = row_ok ? (int)wt : 0;
        pgx_setup(nb, 0.0f, psi, pg_key, (unsigned long long)sw * MT + jt, rec_g[tid], rec_p[tid]);
        pgx_run(&rec_g[tid], &rec_p[tid], 1, &pg_out[tid], 1, 1, [&](int) { return psi; });
        wt = (double)pg_out[tid];
      }
#pragma unroll
      for (int p = 0; p < K; ++p) {
        const double t = wt * v[p];
        acc[KK + p] = fma(y, v[p], acc[KK + p]);
#pragma unroll
        for (int q = 0; q <= p; ++q) acc[lidx(p, q)] = fma(t, v[q], acc[lidx(p, q)]);
      }
    }
    // ---- the parts of a row, added in part order
    for (int p = 1; p < FOLD_PARTS; ++p) {
      __syncthreads();
      if (wv == p) {
#pragma unroll
        for (int e = 0; e < NA; ++e) red[e][lane] = acc[e];
      }
      __syncthreads();
      if (wv == 0) {
#pragma unroll
        for (int e = 0; e < NA; ++e) acc[e] += red[e][lane];
      }
    }
    // ---- solve and draw (factor.py:349-362): wave 0, one row per lane
    if (wv == 0) {
      const double inv_nu2 = (FAM == FOLD_GAUSSIAN && a.noise) ? 1.0 / a.noise[(size_t)s * a.nstride] : 1.0;
      const double inv_s2 = 1.0 / a.sigma2[(size_t)s * a.sstride];
      double L[KK], m[K], u[K];
#pragma unroll
      for (int e = 0; e < KK; ++e) L[e] = acc[e] * inv_nu2;
#pragma unroll
      for (int k = 0; k < K; ++k) { L[lidx(k, k)] += inv_s2; m[k] = acc[KK + k] * inv_nu2; }
      bool ok = true;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        double d = L[lidx(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d = fma(-L[lidx(j, k)], L[lidx(j, k)], d);
        ok = ok && d > 0.0;                                  // (false for nan: a non-finite nu2 / sigma2 / V ends here too)
        const double dj = sqrt(d), rj = 1.0 / dj;
        L[lidx(j, j)] = dj;
#pragma unroll
        for (int i = j + 1; i < K; ++i) {
          double x = L[lidx(i, j)];
#pragma unroll
          for (int k = 0; k < j; ++k) x = fma(-L[lidx(i, k)], L[lidx(j, k)], x);
          L[lidx(i, j)] = x * rj;
        }
      }
      // mean: L y = b, L' m = y
#pragma unroll
      for (int i = 0; i < K; ++i) {
        double x = m[i];
#pragma unroll
        for (int k = 0; k < i; ++k) x = fma(-L[lidx(i, k)], m[k], x);
        m[i] = x / L[lidx(i, i)];
      }
#pragma unroll
      for (int i = K - 1; i >= 0; --i) {
        double x = m[i];
#pragma unroll
        for (int k = i + 1; k < K; ++k) x = fma(-L[lidx(k, i)], m[k], x);
        m[i] = x / L[lidx(i, i)];
      }
      // u = L^-T z
#pragma unroll
      for (int k = 0; k < K; ++k)
        u[k] = a.z ? a.z[((size_t)s * R + rc) * K + k] : philox_normal(a.seed, stream, (unsigned long long)sw * K + k);
#pragma unroll
      for (int i = K - 1; i >= 0; --i) {
        double x = u[i];
#pragma unroll
        for (int k = i + 1; k < K; ++k) x = fma(-L[lidx(k, i)], u[k], x);
        u[i] = x / L[lidx(i, i)];
      }
#pragma unroll
      for (int k = 0; k < K; ++k) w[k] = ok ? m[k] + u[k] : __builtin_nan("");
      if (!ok && row_ok) {
        a.status[0] = 1;
        atomicMin(&a.status[1], (int)(sg * (unsigned long long)R + (unsigned)r));
      }
      if (sw + 1 == nsweeps && row_ok) {
        double* __restrict__ wo = a.W + ((size_t)s * R + r) * K;
#pragma unroll
        for (int k = 0; k < K; ++k) wo[k] = w[k];
        if (a.Wmean) {
          double* __restrict__ mo = a.Wmean + ((size_t)s * R + r) * K;
#pragma unroll
          for (int k = 0; k < K; ++k) mo[k] = ok ? m[k] : __builtin_nan("");
        }
      }
      if (FAM == FOLD_BINOMIAL) {
#pragma unroll
        for (int k = 0; k < K; ++k) wsh[k][lane] = w[k];
      }
    }
    if constexpr (FAM == FOLD_BINOMIAL) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < K; ++k) w[k] = wsh[k][lane];
    }
  }
}

}  // namespace btf
#endif  // BTF_FOLD_UNIT
