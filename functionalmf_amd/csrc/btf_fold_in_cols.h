// Folding new columns into a fitted posterior  (counted under BTF_K_CRITERIA)
//
// Reference: given W the columns of V are conditionally independent (factor.py:378: _resample_V walks them one by one), but
// the prior of a column hangs on horseshoe+ local scales of its own (factor.py:404-405), which nobody has sampled for a NEW
// column.  Given a kept sample's W_s, nu2_s and lam2_s the new column's curve v (T x K, depth-major: index t K + k) and its
// levels (tau2, c, b, a), nD values each, form a small Gibbs chain:
//     start    a = 1 / g0[0], b = 1 / (a g0[1]), c = 1 / (b g0[2]), tau2 = min(1 / (c g0[3]), 9)     g0 ~ Gamma(1/2, 1)
//              (sample_horseshoe_plus with the clip of _init_Tau2)
//     sweep    Q = blockdiag_t(A_t) + Delta' diag(1 / (lam2 tau2)) Delta (x) I_K,  A_t = sum_i cnt_it w_i w_i' / nu2,
//              b_t = sum_i ysum_it w_i / nu2;  Q = L L',  v = Q^-1 b + L^-T z                      (factor.py:378-409)
//              rate = sum_k (Delta v_k)^2 / (2 lam2) + 1 / clip(c),  tau2 = clip(rate) / g[0]      g[0] ~ Gamma((K+1)/2, 1)
//              c = clip(1 / tau2 + 1 / b) / g[1],  b = clip(1 / c + 1 / a) / g[2],  a = clip(1 / b + 1) / g[3]
//                                                                            g[1..3] ~ Gamma(1, 1)  (factor.py:136-141)
// Binomial columns (factor.py:437-460) start at v = 0 and open every sweep with omega_it ~ PG(n_it, w_i . v_t) from the current
// v by the exact sampler of btf_pg_exact.h; A_t = sum_i omega_it w_i w_i' and b_t = sum_i (y_it - n_it / 2) w_i.
// functionalmf_amd/fold_in_cols.py restates this in numpy (`conditional`, `chain`); that module is the definition.
//
// ONE launch, fold_cols_kernel<K, FAMILY>, ONE geometry: a workgroup of one wave owns the chain of (sample s, new column c) for all
// its sweeps; S * C chains in a launch.
//   accumulation   once per chain (Binomial: once per sweep, after its Polya-Gamma draws): for every depth t the lanes walk the N rows (lane l takes rows l, l + 64, ... in
//       ascending order: cnt and ysum lie [column][depth][row], one coalesced load per 64 rows), keep the K (K + 1) / 2 + K
//       running sums of their rows in registers, and the 64 partial sums are added by the xor butterfly - a fixed order
//       that depends on N alone.  A missing cell has cnt = ysum = 0 and adds exact zeros.  A_t and b_t stay in LDS.
//   band           the band of Q in LDS, column nn at B[nn (bw + 1)], half bandwidth bw = (tf + 1) K: within a depth the
//       offsets reach K - 1, across depths the prior couples (t, k) with (t + d, k), d <= tf + 1, at offset d K.  The prior
//       band is formed from 1 / (lam2 tau2) through the Delta' Delta stencil as band_side (btf_kernels.h) does.
//   draw           banded_factor_forward / banded_backward of btf_kernels.h in natural order (one wave, no pivoting): the
//       forward substitution of b rides in the factorisation, then two backward substitutions (mean; L^-T z).  A
//       non-positive pivot sets the chain's outputs to nan, raises the status flag and leaves the smallest failing
//       (global sample) * C + column (integer atomicMin): BTF_ESTATE with btf_fail_index.
//   levels         lane = penalty row, gamma_mt (btf_kernels.h) on a generator of the row.
// Generator: Philox keyed (seed, stream = global sample index << 32 | column, counter = slot << 44 | element << 12 | block)
// with slot 0 the start and slot r + 1 sweep r, element = penalty row for the level draws and nD + coordinate for the
// normals; the Polya-Gamma stream of a cell is keyed by (a Philox word of slot FOLDC_PG_SLOT, (sweep T + t) N + i) - never a
// thread or block index: splitting S over calls (sample0) or folding columns one at a time gives the same
// bits.  `draws` (one flat block per chain, the layout of fold_in_cols.chain) replaces every variate.
// LDS per workgroup: foldc_lds_bytes (41 KB band + 28 KB side arrays at T = 64, K = 5, tf = 2); beyond FOLDC_LDS_LIMIT the
// call is refused - there is no second code path.  fp64 throughout, no floating-point atomics.
#pragma once
#include "btf_device.h"
#include <math.h>

namespace btf {

enum { FOLDC_GAUSSIAN = 0, FOLDC_BINOMIAL = 1 };
constexpr size_t FOLDC_LDS_LIMIT = 156 * 1024;      // what one workgroup may hold of a CU's 160 KiB beside the Polya-Gamma records
constexpr int FOLDC_MAX_TRIALS = 32;                // PG_AUTO_EXACT_MAX: the counts drawn exactly (btf_fold_in.h)
constexpr unsigned long long FOLDC_PG_SLOT = 0xFFFFFULL;   // the generator slot of the Polya-Gamma key: sweeps stay below it
constexpr double FOLDC_TAU2_START_CLIP = 9.0;       // _init_Tau2

struct FoldColsArgs {
  const double* W;          // [S][N][K]
  const double* noise;      // nu2 of sample s at noise[s * nstride] (Gaussian; Binomial: not read)
  const double* lam2;       // lam2 of sample s at lam2[s * lstride]
  const double* cnt;        // [C][T][N] Gaussian: observed replicates of the cell; Binomial: trials (0: missing)
  const double* ysum;       // [C][T][N] Gaussian: sum of the observed replicates; Binomial: kappa = successes - trials / 2
  const double* draws;      // [S][C][4 nD + sweeps (T K + 4 nD)] or null: the device generator
  const int* rcol0;         // [nD] first depth a penalty row touches
  const double* rcoef;      // [nD][tf + 2] its coefficients from there on (0 past the row's end)
  const int* st_ptr;        // [T (tf + 2) + 1] CSR of the Delta' Delta stencil per (t, d): entry (t + d, t) of the prior band
  const int* st_row;
  const double* st_coef;
  double* V;                // [S][C][T][K]
  double* Vmean;            // [S][C][T][K] the last conditional mean
  double* Tau2;             // [S][C][nD]
  int* status;              // [0]: 1 after a non-positive pivot, [1]: the smallest failing (sample0 + s) * C + c
  unsigned long long seed;
  long long sample0;        // global index of sample 0 of this call (generator keys)
  double lo, hi;            // clip: stability, 1 / stability
  int nstride, lstride;
  int S, C, N, T, tf, nD, sweeps;
};

// the same count in fold_in_cols.lds_bytes
inline size_t foldc_lds_bytes(int T, int K, int tf, int nD) {
  const size_t n = (size_t)T * K, bw = (size_t)(tf + 1) * K, npairs = bw * (bw + 1) / 2;
  return 8 * (n * (bw + 1) + 4 * n + (size_t)T * tri(K) + 5 * (size_t)nD + (size_t)T * (tf + 2)) + 8 * ((npairs + 3) / 4);
}

// the kernels live in btf_fold_in_cols.hip (a compilation unit of their own); the C-ABI unit launches them through this
using FoldColsKernel = void (*)(FoldColsArgs);
FoldColsKernel fold_cols_fn(int K, int family);    // null outside K = 1..10, family = 0..1

}  // namespace btf

#ifdef BTF_FOLD_COLS_UNIT
#include "btf_kernels.h"        // banded_factor_forward / banded_backward, fill_pair_table, CellRng, gamma_mt
#include "btf_pg_exact.h"       // pgx_setup / pgx_run

namespace btf {

// the generator of one element of one slot of the chain `stream`
__device__ __forceinline__ CellRng foldc_rng(unsigned long long seed, unsigned long long stream, int slot, int element) {
  CellRng g(seed, stream);
  g.ctr = ((unsigned long long)slot << 44) | ((unsigned long long)(unsigned)element << 12);
  return g;
}

template <int K, int FAM>
__global__ __launch_bounds__(WAVE) void fold_cols_kernel(FoldColsArgs a) {
  constexpr int KK = tri(K), NA = KK + K;
  extern __shared__ double lds[];
  __shared__ uint4 rec_g[FAM == FOLDC_BINOMIAL ? WAVE : 1], rec_p[FAM == FOLDC_BINOMIAL ? WAVE : 1];
  __shared__ float pg_out[FAM == FOLDC_BINOMIAL ? WAVE : 1];
  const int lane = threadIdx.x;
  const int T = a.T, N = a.N, nD = a.nD, D1 = a.tf + 2, n = T * K, bw = (a.tf + 1) * K, R1 = bw + 1;
  const int s = blockIdx.x / a.C, c = blockIdx.x - s * a.C;
  double* B = lds;                      // [n][R1] the band of Q, then of L
  double* rm = B + (size_t)n * R1;      // [n] b -> L^-1 b -> mean
  double* ru = rm + n;                  // [n] z -> L^-T z -> v
  double* invd = ru + n;                // [n] 1 / L_ii
  double* bv = invd + n;                // [n] b
  double* A = bv + n;                   // [T][KK] packed lower triangles of A_t
  double* tau = A + (size_t)T * KK;     // [nD] x 4: tau2, c, b, a
  double* lc = tau + nD;
  double* lb = lc + nD;
  double* la = lb + nD;
  double* itau = la + nD;               // [nD] 1 / (lam2 tau2)
  double* pb = itau + nD;               // [T][D1] the prior band: entry (t + d, t)
  unsigned short* ptab = reinterpret_cast<unsigned short*>(pb + (size_t)T * D1);
  const unsigned long long sg = (unsigned long long)(a.sample0 + s);
  const unsigned long long stream = (sg << 32) | (unsigned long long)(unsigned)c;
  const size_t chain = (size_t)s * a.C + c;
  const size_t LD = (size_t)4 * nD + (size_t)a.sweeps * (n + 4 * nD);
  const double* dr = a.draws ? a.draws + chain * LD : nullptr;
  const double lam2 = a.lam2[(size_t)s * a.lstride];
  const double inv_nu2 = (FAM == FOLDC_GAUSSIAN) ? 1.0 / a.noise[(size_t)s * a.nstride] : 1.0;
  const double lo = a.lo, hi = a.hi;
  auto clip = [&](double x) { return fmin(fmax(x, lo), hi); };

  fill_pair_table(ptab, bw);
  unsigned long long pg_key = 0;
  if constexpr (FAM == FOLDC_BINOMIAL) {
    uint32_t kw[4];
    Philox::gen(a.seed, stream, FOLDC_PG_SLOT << 44, kw);    // a counter the chain's other draws never reach
    pg_key = ((unsigned long long)kw[1] << 32) | kw[0];
    for (int idx = lane; idx < n; idx += WAVE) ru[idx] = 0.0;  // the chain starts at v = 0
    __syncthreads();
  }
  // A_t and b_t, lanes along rows, every depth in turn.  Gaussian: once per chain, A_t = sum cnt w w' / nu2.  Binomial: every
  // sweep, after omega_it ~ PG(n_it, w_i . v_t) from the current v (ru): A_t = sum omega w w', b_t = sum kappa w.
  auto accumulate = [&](int sw) {
    const double* __restrict__ W = a.W + (size_t)s * N * K;
    for (int t = 0; t < T; ++t) {
      const double* __restrict__ cn = a.cnt + ((size_t)c * T + t) * N;
      const double* __restrict__ ys = a.ysum + ((size_t)c * T + t) * N;
      double vt[K];
      if constexpr (FAM == FOLDC_BINOMIAL) {
#pragma unroll
        for (int k = 0; k < K; ++k) vt[k] = ru[t * K + k];
      }
      double acc[NA];
#pragma unroll
      for (int e = 0; e < NA; ++e) acc[e] = 0.0;
      for (int i0 = 0; i0 < N; i0 += WAVE) {               // (every lane of the wave takes part in the Polya-Gamma loop)
        const int i = i0 + lane;
        const bool row_ok = i < N;
        const int ic = row_ok ? i : N - 1;
        double w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = W[(size_t)ic * K + k];
        double cw = row_ok ? cn[ic] : 0.0;
        const double y = row_ok ? ys[ic] : 0.0;
        if constexpr (FAM == FOLDC_BINOMIAL) {
          double psi = 0.0;
#pragma unroll
          for (int k = 0; k < K; ++k) psi = fma(w[k], vt[k], psi);
          pgx_setup((int)cw, 0.0f, psi, pg_key, ((unsigned long long)sw * T + t) * N + ic, rec_g[lane], rec_p[lane]);
          pgx_run(&rec_g[lane], &rec_p[lane], 1, &pg_out[lane], 1, 1, [&](int) { return psi; });
          cw = (double)pg_out[lane];
        }
#pragma unroll
        for (int p = 0; p < K; ++p) {
          const double tw = cw * w[p];
          acc[KK + p] = fma(y, w[p], acc[KK + p]);
#pragma unroll
          for (int q = 0; q <= p; ++q) acc[lidx(p, q)] = fma(tw, w[q], acc[lidx(p, q)]);
        }
      }
#pragma unroll
      for (int e = 0; e < NA; ++e) acc[e] = wave_sum(acc[e]);
      if (lane == 0) {
#pragma unroll
        for (int e = 0; e < KK; ++e) A[(size_t)t * KK + e] = acc[e] * inv_nu2;
#pragma unroll
        for (int k = 0; k < K; ++k) bv[t * K + k] = acc[KK + k] * inv_nu2;
      }
    }
  };
  if constexpr (FAM == FOLDC_GAUSSIAN) accumulate(0);
  // ---- the start of the levels: sample_horseshoe_plus, Tau2 clipped as _init_Tau2 does
  for (int r = lane; r < nD; r += WAVE) {
    double g0[4];
    if (dr) {
#pragma unroll
      for (int j = 0; j < 4; ++j) g0[j] = dr[(size_t)j * nD + r];
    } else {
      CellRng g = foldc_rng(a.seed, stream, 0, r);
#pragma unroll
      for (int j = 0; j < 4; ++j) g0[j] = gamma_mt(0.5, g);
    }
    const double av = 1.0 / g0[0], bq = 1.0 / (av * g0[1]), cv = 1.0 / (bq * g0[2]);
    la[r] = av; lb[r] = bq; lc[r] = cv;
    tau[r] = fmin(1.0 / (cv * g0[3]), FOLDC_TAU2_START_CLIP);
  }
  __syncthreads();

  bool ok = true;
  for (int sw = 0; sw < a.sweeps; ++sw) {
    const double* ds = dr ? dr + (size_t)4 * nD + (size_t)sw * (n + 4 * nD) : nullptr;
    if constexpr (FAM == FOLDC_BINOMIAL) { accumulate(sw); __syncthreads(); }
    // ---- the prior band from 1 / (lam2 tau2)
    for (int r = lane; r < nD; r += WAVE) itau[r] = 1.0 / (lam2 * tau[r]);
    __syncthreads();
    for (int e0 = lane; e0 < T * D1; e0 += WAVE) {
      double sum = 0.0;
      for (int e = a.st_ptr[e0]; e < a.st_ptr[e0 + 1]; ++e) sum = fma(a.st_coef[e], itau[a.st_row[e]], sum);
      pb[e0] = sum;
    }
    __syncthreads();
    // ---- the band of Q: column nn = t K + k holds the entries (nn + off, nn), off = 0..bw
    for (int idx = lane; idx < n * R1; idx += WAVE) {
      const int nn = idx / R1, off = idx - nn * R1;
      const int t = nn / K, k = nn - t * K;
      const int row = nn + off, t2 = row / K, k2 = row - t2 * K;
      double v = 0.0;
      if (row < n) {
        if (t2 == t) v = A[(size_t)t * KK + lidx(k2, k)];
        if (k2 == k) v += pb[t * D1 + (t2 - t)];
      }
      B[idx] = v;
    }
    for (int idx = lane; idx < n; idx += WAVE) {
      rm[idx] = bv[idx];
      double z;
      if (ds) z = ds[idx];
      else { CellRng g = foldc_rng(a.seed, stream, sw + 1, nD + idx); z = g.normal(); }
      ru[idx] = z;
    }
    __syncthreads();
    // ---- Q = L L', rm = L^-1 b; then mean = L^-T rm and u = L^-T z
    ok = banded_factor_forward(B, rm, invd, ptab, n, bw);
    if (!ok) break;
    __syncthreads();
    banded_backward(B, rm, invd, n, bw);
    banded_backward(B, ru, invd, n, bw);
    __syncthreads();
    for (int idx = lane; idx < n; idx += WAVE) ru[idx] += rm[idx];
    __syncthreads();
    // ---- the levels (factor.py:136-141), lane = penalty row
    for (int r = lane; r < nD; r += WAVE) {
      const int t0 = a.rcol0[r];
      double dv[K];
#pragma unroll
      for (int k = 0; k < K; ++k) dv[k] = 0.0;
      for (int e = 0; e < D1; ++e) {
        const double cf = a.rcoef[(size_t)r * D1 + e];
        const int t = min(t0 + e, T - 1);                    // (cf = 0 past the row's end)
#pragma unroll
        for (int k = 0; k < K; ++k) dv[k] = fma(cf, ru[t * K + k], dv[k]);
      }
      double dsq = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) dsq = fma(dv[k], dv[k], dsq);
      double g4[4];
      if (ds) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g4[j] = ds[(size_t)n + (size_t)j * nD + r];
      } else {
        CellRng g = foldc_rng(a.seed, stream, sw + 1, r);
        g4[0] = gamma_mt(0.5 * (K + 1), g);
#pragma unroll
        for (int j = 1; j < 4; ++j) g4[j] = gamma_mt(1.0, g);
      }
      const double rate = dsq / (2.0 * lam2) + 1.0 / clip(lc[r]);
      const double tv = clip(rate) / g4[0];
      const double cv = clip(1.0 / tv + 1.0 / lb[r]) / g4[1];
      const double bq = clip(1.0 / cv + 1.0 / la[r]) / g4[2];
      const double av = clip(1.0 / bq + 1.0) / g4[3];
      tau[r] = tv; lc[r] = cv; lb[r] = bq; la[r] = av;
    }
    __syncthreads();
  }
  // ---- the last state of the chain; nan after a failed factorisation
  const double bad = __builtin_nan("");
  double* __restrict__ Vo = a.V + chain * n;
  double* __restrict__ Mo = a.Vmean + chain * n;
  double* __restrict__ To = a.Tau2 + chain * nD;
  for (int idx = lane; idx < n; idx += WAVE) { Vo[idx] = ok ? ru[idx] : bad; Mo[idx] = ok ? rm[idx] : bad; }
  for (int r = lane; r < nD; r += WAVE) To[r] = ok ? tau[r] : bad;
  if (!ok && lane == 0) {
    a.status[0] = 1;
    atomicMin(&a.status[1], (int)(sg * (unsigned long long)a.C + (unsigned)c));
  }
}

}  // namespace btf
#endif  // BTF_FOLD_COLS_UNIT
