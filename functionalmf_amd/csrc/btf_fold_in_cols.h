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
// Negative-Binomial columns (FOLDC_NEGBIN, instantiated beside the two others for btf_negbin_fold_in_cols alone) are Binomial
// columns with the pseudo-data of factor.py:506-511: omega_it ~ PG(ysum_it + c_it r_it, w_i . v_t) and kappa = (ysum - c r) / 2
// with the rate r read through four strides; their weights are drawn by negbin_accumulate (btf_fold_chain.h), one depth at a
// time through an [N] buffer in LDS; functionalmf_amd/negbin_fold_in.py (`chain_cols`) is their definition.
//
// ONE launch, fold_cols_kernel<K, FAMILY>, ONE geometry: a workgroup of one wave owns the chain of (sample s, new column c) for all
// its sweeps; S * C chains in a launch.  The steps below are those of btf_fold_chain.h (accumulate_blocks, prior_band, fill_band,
// levels_start, levels_update, gibbs_finish), shared with the other three kernels of the family; this kernel's own are the
// Polya-Gamma key, start and weights of the Binomial family.
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
// normals; the Polya-Gamma stream of a cell is keyed by (a Philox word of slot FOLD_CHAIN_PG_SLOT, (sweep T + t) N + i) - never a
// thread or block index: splitting S over calls (sample0) or folding columns one at a time gives the same
// bits.  `draws` (one flat block per chain, the layout of fold_in_cols.chain) replaces every variate.
// LDS per workgroup: foldc_lds_bytes (41 KB band + 28 KB side arrays at T = 64, K = 5, tf = 2), the count of fold_chain_layout;
// beyond FOLDC_LDS_LIMIT the call is refused - there is no second code path.  fp64 throughout, no floating-point atomics.
#pragma once
#include "btf_fold_chain.h"

namespace btf {

enum { FOLDC_GAUSSIAN = 0, FOLDC_BINOMIAL = 1, FOLDC_NEGBIN = 2 };   // (2: btf_negbin_fold_in_cols alone, through fold_cols_negbin_fn)
constexpr size_t FOLDC_LDS_LIMIT = FOLD_CHAIN_LDS_LIMIT;      // (beside the Polya-Gamma records)

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
  // the Negative-Binomial family alone (cnt: observed replicates, ysum: their sum)
  const double* rate;       // the rate of (sample s, column c, row i, depth t) at rate[s rs_s + c rs_c + i rs_i + t rs_t]
  const double* omega;      // [S][C][sweeps][T][N] weights in the place of every Polya-Gamma draw, or null
  long long rs_s, rs_c, rs_i, rs_t;   // 0 on an axis the rate is shared along
};

// the same count in fold_in_cols.lds_bytes: 8 (n (bw + 1) + 4 n + T K (K + 1) / 2 + 5 nD + T (tf + 2)) + the pair table
inline size_t foldc_lds_bytes(int T, int K, int tf, int nD) { return fold_chain_lds_bytes(T, K, tf, (tf + 1) * K, nD, 0, false); }
// the Negative-Binomial family: + 8 N for the weights of one depth (negbin_fold_in.lds_bytes)
inline size_t foldc_negbin_lds_bytes(int T, int K, int tf, int nD, int N) { return fold_chain_lds_bytes(T, K, tf, (tf + 1) * K, nD, 0, false, N); }

// the kernels live in btf_fold_in_cols.hip (a compilation unit of their own); the C-ABI unit launches them through this
using FoldColsKernel = void (*)(FoldColsArgs);
FoldColsKernel fold_cols_fn(int K, int family);    // null outside K = 1..10, family = 0..1
FoldColsKernel fold_cols_negbin_fn(int K);         // the Negative-Binomial family (btf_negbin_fold_in_cols); null outside K = 1..10

}  // namespace btf

#ifdef BTF_FOLD_COLS_UNIT
#include "btf_pg_exact.h"       // pgx_setup / pgx_run

namespace btf {

template <int K, int FAM>
__global__ __launch_bounds__(WAVE) void fold_cols_kernel(FoldColsArgs a) {
  extern __shared__ double lds[];
  __shared__ uint4 rec_g[FAM == FOLDC_BINOMIAL ? WAVE : 1], rec_p[FAM == FOLDC_BINOMIAL ? WAVE : 1];
  __shared__ float pg_out[FAM == FOLDC_BINOMIAL ? WAVE : 1];
  const int lane = threadIdx.x;
  const int T = a.T, N = a.N, nD = a.nD, D1 = a.tf + 2, n = T * K, bw = (a.tf + 1) * K;
  const int s = blockIdx.x / a.C, c = blockIdx.x - s * a.C;
  FoldChainLds m;
  fold_chain_layout(m, lds, T, K, a.tf, bw, nD, 0, false, FAM == FOLDC_NEGBIN ? N : 0);
  const unsigned long long sg = (unsigned long long)(a.sample0 + s);
  const unsigned long long stream = (sg << 32) | (unsigned long long)(unsigned)c;
  const size_t chain = (size_t)s * a.C + c;
  const size_t LD = (size_t)4 * nD + (size_t)a.sweeps * (n + 4 * nD);
  const double* dr = a.draws ? a.draws + chain * LD : nullptr;
  const double lam2 = a.lam2[(size_t)s * a.lstride];
  const double* __restrict__ W = a.W + (size_t)s * N * K;
  const double* cn = a.cnt + (size_t)c * T * N;
  const double* ys = a.ysum + (size_t)c * T * N;

  fill_pair_table(m.ptab, bw);
  unsigned long long pg_key = 0;
  if constexpr (FAM != FOLDC_GAUSSIAN) {
    uint32_t kw[4];
    Philox::gen(a.seed, stream, FOLD_CHAIN_PG_SLOT << 44, kw);    // a counter the chain's other draws never reach
    pg_key = ((unsigned long long)kw[1] << 32) | kw[0];
    for (int idx = lane; idx < n; idx += WAVE) m.ru[idx] = 0.0;  // the chain starts at v = 0
    __syncthreads();
  }
  // Gaussian: A_t = sum cnt w w' / nu2, once per chain.  Binomial: every sweep, after omega_it ~ PG(n_it, w_i . v_t) from the
  // current v (ru): A_t = sum omega w w', b_t = sum kappa w.
  if constexpr (FAM == FOLDC_GAUSSIAN) accumulate_blocks<K>(m.A, m.bv, lane, W, cn, ys, T, N, 1.0 / a.noise[(size_t)s * a.nstride], CellWeight());
  levels_start(m, lane, nD, dr, nullptr, a.seed, stream);
  __syncthreads();

  bool ok = true;
  for (int sw = 0; sw < a.sweeps; ++sw) {
    const double* ds = dr ? dr + (size_t)4 * nD + (size_t)sw * (n + 4 * nD) : nullptr;
    if constexpr (FAM == FOLDC_BINOMIAL) {
      accumulate_blocks<K>(m.A, m.bv, lane, W, cn, ys, T, N, 1.0, [&](int t, int i, const double (&w)[K], double trials) {
        double psi = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) psi = fma(w[k], m.ru[t * K + k], psi);
        pgx_setup((int)trials, 0.0f, psi, pg_key, ((unsigned long long)sw * T + t) * N + i, rec_g[lane], rec_p[lane]);
        pgx_run(&rec_g[lane], &rec_p[lane], 1, &pg_out[lane], 1, 1, [&](int) { return psi; });
        return (double)pg_out[lane];
      });
      __syncthreads();
    }
    if constexpr (FAM == FOLDC_NEGBIN) {                 // omega_it ~ PG(ysum + c r, w_i . v_t), kappa = (ysum - c r) / 2
      const NegbinRate nb = {a.rate + (size_t)s * a.rs_s + (size_t)c * a.rs_c, a.rs_i, a.rs_t,
                             a.omega ? a.omega + (chain * a.sweeps + sw) * (size_t)T * N : nullptr};
      negbin_accumulate<K>(m, lane, W, cn, ys, m.ru, T, N, nb, pg_key, sw);
    }
    prior_band(m, lane, nD, T * D1, lam2, a.st_ptr, a.st_row, a.st_coef);
    fill_band<K>(m, lane, n, bw, D1);
    sweep_normals(m, lane, n, nD, ds, a.seed, stream, sw + 1, true);       // (and rm = b)
    __syncthreads();
    // ---- Q = L L', rm = L^-1 b; then mean = L^-T rm and u = L^-T z
    ok = banded_factor_forward(m.B, m.rm, m.invd, m.ptab, n, bw);
    if (!ok) break;
    __syncthreads();
    banded_backward(m.B, m.rm, m.invd, n, bw);
    banded_backward(m.B, m.ru, m.invd, n, bw);
    __syncthreads();
    for (int idx = lane; idx < n; idx += WAVE) m.ru[idx] += m.rm[idx];
    __syncthreads();
    levels_update<K, false>(m, lane, m.ru, nullptr, nD, T, D1, a.rcol0, a.rcoef, ds, (size_t)n, lam2, a.lo, a.hi, a.seed, stream, sw + 1);
    __syncthreads();
  }
  gibbs_finish(m, lane, n, nD, ok, a.V + chain * n, a.Vmean + chain * n, a.Tau2 + chain * nD, a.status,
               (int)(sg * (unsigned long long)a.C + (unsigned)c));
}

}  // namespace btf
#endif  // BTF_FOLD_COLS_UNIT
