// Folding new depth slices into a fitted posterior  (counted under BTF_K_CRITERIA)
//
// The trend-filtering prior of a column couples a new depth with the last tf + 1 kept depths of that column through penalty
// rows whose horseshoe+ local scales nobody has sampled.  With D' the operator on T + H points, R its rows with a non-zero at a
// new depth (nR of them) and D'[R] = [D_o | D_n], the H new depths v (H x K, depth-major: index t K + k) of column j under kept
// sample s and the levels (tau2, c, b, a) of the rows of R form a small Gibbs chain given W_s, V_s[j], nu2_s and lam2_s:
//     start    a = 1 / g0[0], b = 1 / (a g0[1]), c = 1 / (b g0[2]), tau2 = min(1 / (c g0[3]), 9)     g0 ~ Gamma(1/2, 1)
//     sweep    off = D_o V_s[j] (nR x K);  Q = blockdiag_t(A_t) + D_n' diag(1 / (lam2 tau2)) D_n (x) I_K,
//              rhs = b - vec(D_n' diag(1 / (lam2 tau2)) off);  Q = L L',  v = Q^-1 rhs + L^-T z
//              dv = off + D_n v,  rate = sum_k dv_k^2 / (2 lam2) + 1 / clip(c),  tau2 = clip(rate) / g[0]   g[0] ~ Gamma((K+1)/2, 1)
//              c = clip(1 / tau2 + 1 / b) / g[1],  b = clip(1 / c + 1 / a) / g[2],  a = clip(1 / b + 1) / g[3]   g[1..3] ~ Gamma(1, 1)
// with A_t = sum_i cnt_it w_i w_i' / nu2 and b_t = sum_i ysum_it w_i / nu2 (Gaussian).  Binomial slices start at v_t = V_s[j, T - 1]
// for every new t and open every sweep with omega_it ~ PG(n_it, w_i . v_t) from the current v by the exact sampler of
// btf_pg_exact.h; A_t = sum_i omega_it w_i w_i' and b_t = sum_i (y_it - n_it / 2) w_i.  A slice without any observation is
// allowed (D_n has full column rank): the forecast.  Rows of D' on kept depths alone drop out, so no kept Tau2 is read.
// functionalmf_amd/fold_in_depth.py restates this in numpy (`conditional`, `chain`); that module is the definition.
// Negative-Binomial slices (FOLDD_NEGBIN, instantiated beside the two others for btf_negbin_fold_in_depth alone) are Binomial
// slices with omega_it ~ PG(ysum_it + c_it r_it, w_i . v_t) and kappa = (ysum - c r) / 2 (negbin_accumulate, btf_fold_chain.h);
// functionalmf_amd/negbin_fold_in.py (`chain_depth`) is their definition.
//
// ONE launch, fold_depth_kernel<K, FAMILY>, ONE geometry: a workgroup of one wave owns the chain of (sample s, fitted column j)
// for all its sweeps; S * M chains in a launch - the geometry of fold_cols_kernel (btf_fold_in_cols.h); accumulation, band,
// offsets and levels are the steps of btf_fold_chain.h on a system H K wide, and this kernel's own are the start of the
// Binomial chain at the last kept depth and its Polya-Gamma weights:
//   kept curve     only the last L = min(T, tf + 1) depths of V_s[j] are read, once, into LDS; off follows from them.
//   accumulation   once per chain (Binomial: once per sweep, after its Polya-Gamma draws): for every new depth the lanes walk
//       the N rows (lane l takes rows l, l + 64, ...: cnt and ysum lie [column][depth][row]), keep the K (K + 1) / 2 + K
//       running sums in registers, and the 64 partial sums are added by the xor butterfly - a fixed order that depends on N
//       alone.  A missing cell has cnt = ysum = 0 and adds exact zeros.
//   band           column nn of Q at B[nn (bw + 1)], half bandwidth bw = min((tf + 1) K, H K - 1): for H <= tf + 1 the system
//       is narrower than the band of the prior and the whole lower triangle is kept.
//   draw           banded_factor_forward / banded_backward of btf_kernels.h in natural order.  A non-positive pivot sets the
//       chain's outputs to nan, raises the status flag and leaves the smallest failing (global sample) * M + column (integer
//       atomicMin): BTF_ESTATE with btf_fail_index.
//   levels         lane = new penalty row, gamma_mt (btf_kernels.h) on a generator of the row.
// Generator: Philox keyed (seed, stream = global sample index << 32 | column, counter = slot << 44 | element << 12 | block)
// with slot 0 the start and slot r + 1 sweep r, element = row of R for the level draws and nR + coordinate for the normals;
// the Polya-Gamma stream of a cell is keyed by (a Philox word of slot FOLD_CHAIN_PG_SLOT, (sweep H + t) N + i) - never a thread or
// block index: splitting S over calls (sample0) gives the same bits.  `draws` (one flat block per chain, the layout of
// fold_in_depth.chain) replaces every variate.
// LDS per workgroup: foldd_lds_bytes (10.1 KB at H = 8, K = 5, tf = 2), the count of fold_chain_layout; beyond FOLDD_LDS_LIMIT
// the call is refused - there is no second code path.  fp64 throughout, no floating-point atomics.
#pragma once
#include "btf_fold_chain.h"

namespace btf {

enum { FOLDD_GAUSSIAN = 0, FOLDD_BINOMIAL = 1, FOLDD_NEGBIN = 2 };   // (2: btf_negbin_fold_in_depth alone, through fold_depth_negbin_fn)
constexpr size_t FOLDD_LDS_LIMIT = FOLD_CHAIN_LDS_LIMIT;      // (beside the Polya-Gamma records)
constexpr int FOLDD_MAX_GRID = 8192;                // ndepth + horizon: the penalty on the extended grid is built dense on the host

struct FoldDepthArgs {
  const double* W;          // [S][N][K]
  const double* Vtail;      // the last L kept depths of V_s[j] at Vtail[(s * M + j) * vstride], [L][K]
  const double* noise;      // nu2 of sample s at noise[s * nstride] (Gaussian; Binomial: not read)
  const double* lam2;       // lam2 of sample s at lam2[s * lstride]
  const double* cnt;        // [M][H][N] Gaussian: observed replicates of the cell; Binomial: trials (0: missing)
  const double* ysum;       // [M][H][N] Gaussian: sum of the observed replicates; Binomial: kappa = successes - trials / 2
  const double* draws;      // [S][M][4 nR + sweeps (H K + 4 nR)] or null: the device generator
  const int* rcol0;         // [nR] first depth a new row touches, counted from the first NEW depth (negative: a kept depth)
  const double* rcoef;      // [nR][tf + 2] its coefficients from there on (0 past the row's end)
  const int* st_ptr;        // [H (tf + 2) + 1] CSR of the D_n' D_n stencil per (t, d): entry (t + d, t) of the prior band
  const int* st_row;
  const double* st_coef;
  double* V;                // [S][M][H][K]
  double* Vmean;            // [S][M][H][K] the last conditional mean
  double* Tau2;             // [S][M][nR]
  int* status;              // [0]: 1 after a non-positive pivot, [1]: the smallest failing (sample0 + s) * M + j
  unsigned long long seed;
  long long sample0;        // global index of sample 0 of this call (generator keys)
  long long vstride;        // doubles between the tails of consecutive (sample, column) pairs
  double lo, hi;            // clip: stability, 1 / stability
  int nstride, lstride;
  int S, M, N, H, L, tf, nR, sweeps;
  // the Negative-Binomial family alone (cnt: observed replicates, ysum: their sum)
  const double* rate;       // the rate of (sample s, column j, row i, new depth t) at rate[s rs_s + j rs_c + i rs_i + t rs_t]
  const double* omega;      // [S][M][sweeps][H][N] weights in the place of every Polya-Gamma draw, or null
  long long rs_s, rs_c, rs_i, rs_t;   // 0 on an axis the rate is shared along
};

// the same count in fold_in_depth.lds_bytes: foldc_lds_bytes on H depths + 8 (nR K + L K) for the offsets and the tail
inline size_t foldd_lds_bytes(int H, int K, int tf, int nR, int L) {
  return fold_chain_lds_bytes(H, K, tf, fold_depth_bandwidth(H, K, tf), nR, L, false);
}
// the Negative-Binomial family: + 8 N for the weights of one depth (negbin_fold_in.lds_bytes)
inline size_t foldd_negbin_lds_bytes(int H, int K, int tf, int nR, int L, int N) {
  return fold_chain_lds_bytes(H, K, tf, fold_depth_bandwidth(H, K, tf), nR, L, false, N);
}

// the kernels live in btf_fold_in_depth.hip (a compilation unit of their own); the C-ABI unit launches them through this
using FoldDepthKernel = void (*)(FoldDepthArgs);
FoldDepthKernel fold_depth_fn(int K, int family);    // null outside K = 1..10, family = 0..1
FoldDepthKernel fold_depth_negbin_fn(int K);         // the Negative-Binomial family (btf_negbin_fold_in_depth); null outside K = 1..10

}  // namespace btf

#ifdef BTF_FOLD_DEPTH_UNIT
#include "btf_pg_exact.h"       // pgx_setup / pgx_run

namespace btf {

template <int K, int FAM>
__global__ __launch_bounds__(WAVE) void fold_depth_kernel(FoldDepthArgs a) {
  extern __shared__ double lds[];
  __shared__ uint4 rec_g[FAM == FOLDD_BINOMIAL ? WAVE : 1], rec_p[FAM == FOLDD_BINOMIAL ? WAVE : 1];
  __shared__ float pg_out[FAM == FOLDD_BINOMIAL ? WAVE : 1];
  const int lane = threadIdx.x;
  const int H = a.H, N = a.N, nR = a.nR, L = a.L, D1 = a.tf + 2, n = H * K, bw = fold_depth_bandwidth(H, K, a.tf);
  const int s = blockIdx.x / a.M, j = blockIdx.x - s * a.M;
  FoldChainLds m;
  fold_chain_layout(m, lds, H, K, a.tf, bw, nR, L, false, FAM == FOLDD_NEGBIN ? N : 0);
  const unsigned long long sg = (unsigned long long)(a.sample0 + s);
  const unsigned long long stream = (sg << 32) | (unsigned long long)(unsigned)j;
  const size_t chain = (size_t)s * a.M + j;
  const size_t LD = (size_t)4 * nR + (size_t)a.sweeps * (n + 4 * nR);
  const double* dr = a.draws ? a.draws + chain * LD : nullptr;
  const double lam2 = a.lam2[(size_t)s * a.lstride];
  const double* __restrict__ W = a.W + (size_t)s * N * K;
  const double* cn = a.cnt + (size_t)j * H * N;
  const double* ys = a.ysum + (size_t)j * H * N;

  fill_pair_table(m.ptab, bw);
  tail_offsets<K>(m, lane, a.Vtail + chain * (size_t)a.vstride, L, nR, D1, a.rcol0, a.rcoef);
  unsigned long long pg_key = 0;
  if constexpr (FAM != FOLDD_GAUSSIAN) {
    uint32_t kw[4];
    Philox::gen(a.seed, stream, FOLD_CHAIN_PG_SLOT << 44, kw);    // a counter the chain's other draws never reach
    pg_key = ((unsigned long long)kw[1] << 32) | kw[0];
    for (int idx = lane; idx < n; idx += WAVE) m.ru[idx] = m.vt[(L - 1) * K + idx % K];   // the chain starts at the last kept depth
  }
  __syncthreads();
  // Gaussian: A_t = sum cnt w w' / nu2 for every new depth, once per chain.  Binomial: every sweep, after omega_it ~
  // PG(n_it, w_i . v_t) from the current v (ru): A_t = sum omega w w', b_t = sum kappa w.
  if constexpr (FAM == FOLDD_GAUSSIAN) accumulate_blocks<K>(m.A, m.bv, lane, W, cn, ys, H, N, 1.0 / a.noise[(size_t)s * a.nstride], CellWeight());
  levels_start(m, lane, nR, dr, nullptr, a.seed, stream);
  __syncthreads();

  bool ok = true;
  for (int sw = 0; sw < a.sweeps; ++sw) {
    const double* ds = dr ? dr + (size_t)4 * nR + (size_t)sw * (n + 4 * nR) : nullptr;
    if constexpr (FAM == FOLDD_BINOMIAL) {
      accumulate_blocks<K>(m.A, m.bv, lane, W, cn, ys, H, N, 1.0, [&](int t, int i, const double (&w)[K], double trials) {
        double psi = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) psi = fma(w[k], m.ru[t * K + k], psi);
        pgx_setup((int)trials, 0.0f, psi, pg_key, ((unsigned long long)sw * H + t) * N + i, rec_g[lane], rec_p[lane]);
        pgx_run(&rec_g[lane], &rec_p[lane], 1, &pg_out[lane], 1, 1, [&](int) { return psi; });
        return (double)pg_out[lane];
      });
      __syncthreads();
    }
    if constexpr (FAM == FOLDD_NEGBIN) {                 // omega_it ~ PG(ysum + c r, w_i . v_t), kappa = (ysum - c r) / 2
      const NegbinRate nb = {a.rate + (size_t)s * a.rs_s + (size_t)j * a.rs_c, a.rs_i, a.rs_t,
                             a.omega ? a.omega + (chain * a.sweeps + sw) * (size_t)H * N : nullptr};
      negbin_accumulate<K>(m, lane, W, cn, ys, m.ru, H, N, nb, pg_key, sw);
    }
    prior_band(m, lane, nR, H * D1, lam2, a.st_ptr, a.st_row, a.st_coef);
    fill_band<K>(m, lane, n, bw, D1);
    rhs_minus_offsets<K>(m, lane, n, nR, D1, a.rcol0, a.rcoef);
    sweep_normals(m, lane, n, nR, ds, a.seed, stream, sw + 1);
    __syncthreads();
    // ---- Q = L L', rm = L^-1 rhs; then mean = L^-T rm and u = L^-T z
    ok = banded_factor_forward(m.B, m.rm, m.invd, m.ptab, n, bw);
    if (!ok) break;
    __syncthreads();
    banded_backward(m.B, m.rm, m.invd, n, bw);
    banded_backward(m.B, m.ru, m.invd, n, bw);
    __syncthreads();
    for (int idx = lane; idx < n; idx += WAVE) m.ru[idx] += m.rm[idx];
    __syncthreads();
    levels_update<K, true>(m, lane, m.ru, m.off, nR, H, D1, a.rcol0, a.rcoef, ds, (size_t)n, lam2, a.lo, a.hi, a.seed, stream, sw + 1);
    __syncthreads();
  }
  gibbs_finish(m, lane, n, nR, ok, a.V + chain * n, a.Vmean + chain * n, a.Tau2 + chain * nR, a.status,
               (int)(sg * (unsigned long long)a.M + (unsigned)j));
}

}  // namespace btf
#endif  // BTF_FOLD_DEPTH_UNIT
