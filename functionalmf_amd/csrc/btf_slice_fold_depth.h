// Folding new depth slices into a slice-sampled fit  (counted under BTF_K_CRITERIA)
//
// The sixth cell of the fold-in family: the prior side of btf_fold_in_depth.h (the new penalty rows R of the operator on
// T + H points, D'[R] = [D_o | D_n], offsets off = D_o V_s[j] from the kept tail, fresh horseshoe+ levels) with the curve
// update of btf_slice_fold_cols.h (one elliptical slice update on an ellipse CENTRED on a per-cell Gaussian fit of the
// likelihood).  Given a kept sample's W_s, V_s[j] and lam2_s the H new depths v (H x K, depth-major: index h K + k) of
// fitted column j and the levels of the rows of R form a small chain:
//     fit      per new cell a_ih = 1 / Sigma_fit^2 and a_ih Mu_fit (0: no fit);  A_h = sum_i a_ih w_i w_i', b_h = sum_i a_ih Mu_ih w_i
//              Q = blockdiag_h(A_h) + D_n' diag(1 / (lam2 tau2)) D_n (x) I_K,  m = Q^-1 (b - vec(D_n' diag(1 / (lam2 tau2)) off))
//     sweep    Q = L L', nu = L^-T z;  hh = r(v) + log u_h, phi = 2 pi u_a, bracket [phi - 2 pi, phi];  propose
//              v' = m + (v - m) cos phi + nu sin phi, accept when v' is feasible and r(v') >= hh, else shrink the bracket
//              towards 0; after max_rounds proposals the sweep keeps v and is counted
//              r(v) = loglik(v) + sum_cells eta (a eta / 2 - a Mu),  eta_ih = w_i . v_h
//     feasible sum_t A_o[q,t] (w_i . V_s[j, T - B + t]) + sum_h A_n[q,h] (w_i . v_h) >= c[q] for EVERY fitted row i and every
//              constraint q that touches a new depth; B = the trailing kept depths those rows reach (0: none).  This is the one
//              new ingredient: a constraint may couple a new depth with kept ones (v_{T-1} - v_T >= -1e-2).
//     levels   dv = off + D_n v, levels_update of btf_fold_chain.h; skipped when tau2 is given (held fixed)
// functionalmf_amd/slice_fold_in_depth.py restates the chain in numpy; that module is the definition.
//
// ONE launch, slice_fold_depth_kernel<K, LINK>, ONE geometry (slice_fold_cols_kernel's): a workgroup of one wave owns the
// chain of (sample s, fitted column j) for all its sweeps; S * M chains in a launch.  Tail, accumulation, band, offsets, levels,
// the slice update and the epilogues are the steps of btf_fold_chain.h; this kernel's own are the staged tables, the start at
// the last kept depth, `feasible` with its kept-depth terms and `ratio`.
//   kept tail          the last Lt = max(min(T, tf + 1), B) depths of V_s[j] are read once into LDS; off follows from them.
//   fit accumulation   once per chain: for every new depth the lanes walk the N rows (lane l takes rows l, l + 64, ...; the
//       statistics lie [column][depth][row]: coalesced), the 64 partial sums are added by the xor butterfly - a fixed order
//       that depends on N alone.  A_h, b_h stay in LDS.
//   band, draw         prior_band, fill_band: the band of the H K-wide Q in LDS (half bandwidth min((tf + 1) K, H K - 1)),
//       banded_factor_forward / banded_backward of btf_kernels.h in natural order.  With tau2 fixed Q is factored once.  A
//       non-positive pivot sets the chain's outputs to nan and raises status[2] with the smallest failing
//       (global sample) * M + column in status[3].
//   feasibility        lanes over the N fitted rows, the reduced constraints by their CSR non-zeros over the B + H local depths
//       (local depth l < B: kept depth T - B + l, in the LDS tail; else new depth l - B), a wave vote; tested first: an
//       infeasible proposal costs no likelihood pass.  The kept part of every slack is RECOMPUTED per proposal (no table of
//       N * Jn doubles, no scratch): the terms of a slack are added in ascending depth order by fma, and kept and new eta go
//       through ONE dot-product routine, so a new depth that carries the bits of V_s[j, T - 1] ties exactly: a row (+1, -1)
//       against bound 0 evaluates to exactly 0 and passes >=.
//   likelihood and fit lanes over (new depth, listed row): the host passes, per fitted column, the ascending list of rows that
//       have an observed or fitted cell; poisson_term<LINK> / gg_term on the LDS tables, staged before the first barrier;
//       wave_sum: the same bits in every lane.
//   levels             lane = row of R, gamma_mt.
//   bad start          infeasible, or a non-finite r: nan for that chain, status[0], and the smallest failing index in
//       status[1]; the chain does not run.
// Generator: Philox keyed (seed, stream = global sample index << 32 | fitted column, counter = slot << 44 | element << 12 |
// block), slot 0 the start and slot r + 1 sweep r; element = row of R for the level draws, nR + coordinate for the normals,
// nR + H K + position for u_h, u_a and the shrink uniforms - never a thread or block index: the result does not depend on
// the grid, on how S is split over calls (sample0) or on where the states come from.  `draws` (one flat block per chain, the
// layout of slice_fold_in_depth.chain) replaces every variate.
// LDS per workgroup: sdepth_lds_bytes (18.4 KB at H = 8, K = 5, tf = 2, B = 1 with the static tables); beyond
// SDEPTH_LDS_LIMIT the call is refused - there is no second code path.
// fp64 throughout, no floating-point atomics, no spin-waits, no communication between workgroups.
// Resources per instantiation (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), VGPR by K = 1..10; no
// instantiation uses scratch (0 bytes / lane), 106 SGPR each, AGPR 0 except 16 at K = 10:
//   log link (static LDS 2048 B)         162 162 164 166 168 170 172 187 227 256
//   identity link (2048 B)               154 154 156 158 160 162 164 187 227 256
//   generic: families 2..4 (0 B)         162 162 164 166 168 170 172 187 228 256
//   gamma grid (8192 B)                  169 168 170 172 174 176 178 187 227 256
// One-wave workgroups: a CU holds as many chains as its LDS allows (eight at 18.4 KB), so the register count does not bound
// the occupancy below K = 10.
#pragma once
#include "btf_fold_chain.h"
#include "btf_gamma_grid.h"

namespace btf {

constexpr size_t SDEPTH_LDS_LIMIT = FOLD_CHAIN_LDS_LIMIT;
constexpr size_t SDEPTH_STATIC_LDS = 2 * LOGTAB_N * sizeof(double2) + GG_MAXG * sizeof(GgComp);   // the tables (gamma grid: all three)

struct SliceFoldDepthArgs {
  const double* W;          // [S][N][K]
  const double* Vtail;      // the last Lt kept depths of V_s[j] at Vtail[(s * M + j) * vstride], [Lt][K]
  const double* lam2;       // lam2 of sample s at lam2[s * lstride]
  const double* start;      // [S][M][H][K], or null: every new depth starts at the last kept depth
  const double* S1; const double* cnt; const double* L;    // [M][H][N]; L: gamma grid only
  const double* fa; const double* fb;          // [M][H][N] the fit: a = 1 / Sigma^2, a Mu (0, 0: no fit)
  const int* rptr; const int* ridx;            // [M + 1], rows of column j with an observed or fitted new cell, ascending
  const int* cs_ptr; const int* cs_idx; const double* cs_val; const double* Cc; int J;   // reduced constraints, CSR over [J][B + H]
  const double* tau2;       // [S][M][nR] local scales held fixed, or null: sampled
  const double* draws;      // [S][M][4 nR + sweeps (H K + 1 + max_rounds + 4 nR)] or null: the device generator
  const int* rcol0;         // [nR] first depth a new row touches, counted from the first NEW depth (negative: a kept depth)
  const double* rcoef;      // [nR][tf + 2] its coefficients from there on (0 past the row's end)
  const int* st_ptr;        // [H (tf + 2) + 1] CSR of the D_n' D_n stencil per (h, d): entry (h + d, h) of the prior band
  const int* st_row;
  const double* st_coef;
  const GgComp* gg; int G; double lsp;         // gamma grid: the component table
  int fam; double par;                         // ESS_LINK_GENERIC: the family and its parameter
  double* V;                // [S][M][H][K]
  double* Vstart;           // [S][M][H][K] the start of every chain
  double* Tau2;             // [S][M][nR]
  int* rounds; int* unfinished;                // [S][M]
  int* status;              // [0]: 1 after a bad start, [1]: its smallest (sample0 + s) * M + j; [2], [3]: the same for a pivot
  unsigned long long seed;
  long long sample0;        // global index of sample 0 of this call (generator keys)
  long long vstride;        // doubles between the tails of consecutive (sample, column) pairs
  double lo, hi;            // clip: stability, 1 / stability
  int lstride;
  int S, M, N, H, Lt, B, tf, nR, sweeps, max_rounds;
};

// the same count in slice_fold_in_depth.lds_bytes (dynamic part + the static tables): foldd_lds_bytes with six H K vectors
// (v, m, nu, v', b, the pivots) and the tail of Lt = max(min(T, tf + 1), B) kept depths
inline size_t sdepth_dyn_lds_bytes(int H, int K, int tf, int nR, int Lt) {
  return fold_chain_lds_bytes(H, K, tf, fold_depth_bandwidth(H, K, tf), nR, Lt, true);
}
inline size_t sdepth_lds_bytes(int H, int K, int tf, int nR, int Lt) { return sdepth_dyn_lds_bytes(H, K, tf, nR, Lt) + SDEPTH_STATIC_LDS; }

// the kernels live in btf_slice_fold_depth.hip (a compilation unit of their own); the C-ABI unit launches them through this
using SliceFoldDepthKernel = void (*)(SliceFoldDepthArgs);
SliceFoldDepthKernel slice_fold_depth_fn(int K, int family);     // null outside K = 1..10, family = 0..5 (ESS_FAM_*)

}  // namespace btf

#ifdef BTF_SLICE_FOLD_DEPTH_UNIT
namespace btf {

template <int K, int LINK>
__global__ __launch_bounds__(WAVE) void slice_fold_depth_kernel(SliceFoldDepthArgs a) {
  constexpr bool GG = LINK == ESS_LINK_GAMMA_GRID;
  extern __shared__ double lds[];
  __shared__ double2 ltab[LINK == ESS_LINK_GENERIC ? 1 : LOGTAB_N];
  __shared__ double2 etab[GG ? LOGTAB_N : 1];
  __shared__ GgComp tab[GG ? GG_MAXG : 1];
  if constexpr (GG) gg_stage(GgTab{nullptr, a.gg, a.G, a.lsp}, tab, ltab, etab);
  else if constexpr (LINK == ESS_LINK_IDENTITY) log_table_build(ltab);
  else if constexpr (LINK == ESS_LINK_LOG) exp_table_build(ltab);
  const int lane = threadIdx.x;
  const int H = a.H, N = a.N, nR = a.nR, Lt = a.Lt, NB = a.B, D1 = a.tf + 2, n = H * K, bw = fold_depth_bandwidth(H, K, a.tf);
  const int s = blockIdx.x / a.M, j = blockIdx.x - s * a.M;
  FoldChainLds m;
  fold_chain_layout(m, lds, H, K, a.tf, bw, nR, Lt, true);
  const unsigned long long sg = (unsigned long long)(a.sample0 + s);
  const unsigned long long stream = (sg << 32) | (unsigned long long)(unsigned)j;
  const size_t chain = (size_t)s * a.M + j;
  const int per = n + 1 + a.max_rounds + 4 * nR;                      // one sweep's record
  const size_t LD = (size_t)4 * nR + (size_t)a.sweeps * per;
  const double* dr = a.draws ? a.draws + chain * LD : nullptr;
  const double lam2 = a.lam2[(size_t)s * a.lstride];
  const bool fixed = a.tau2 != nullptr;
  const LikFam lf{a.fam, a.par};
  const double* __restrict__ W = a.W + (size_t)s * N * K;
  const size_t col = (size_t)j * H * N;                                // this column's statistics
  const int* __restrict__ rows = a.ridx + a.rptr[j];
  const int nr = a.rptr[j + 1] - a.rptr[j];

  fill_pair_table(m.ptab, bw);
  tail_offsets<K>(m, lane, a.Vtail + chain * (size_t)a.vstride, Lt, nR, D1, a.rcol0, a.rcoef);
  // ---- A_h and b_h of the fit, then the start: the levels (or the fixed scales) and v
  accumulate_blocks<K>(m.A, m.bv, lane, W, a.fa + col, a.fb + col, H, N, 1.0, CellWeight());
  levels_start(m, lane, nR, dr, fixed ? a.tau2 + chain * nR : nullptr, a.seed, stream);
  {
    const double* __restrict__ st = a.start ? a.start + chain * (size_t)n : nullptr;
    double* __restrict__ V0 = a.Vstart + chain * (size_t)n;
    for (int idx = lane; idx < n; idx += WAVE) {
      const double x = st ? st[idx] : m.vt[(Lt - 1) * K + idx % K];        // (the last kept depth, bit for bit)
      m.xv[idx] = x;
      V0[idx] = x;
    }
  }
  __syncthreads();

  // eta = w_i . x for the row in registers and one depth x[0..K) in LDS: THE dot product of kept and new depths alike
  auto dot = [&](const double (&w)[K], const double* x) {
    double e = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) e = fma(w[k], x[k], e);
    return e;
  };
  // every restriction holds at x (a wave vote; NaN fails every comparison).  Local depth l < NB is kept depth T - NB + l
  // (tail row Lt - NB + l), l >= NB the new depth l - NB; the CSR lists a row's depths in ascending order.
  auto feasible = [&](const double* x) -> bool {
    bool ok = true;
    if (a.J > 0) {
      const double* kept = m.vt + (size_t)(Lt - NB) * K;
      for (int i = lane; i < N; i += WAVE) {
        double w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = W[(size_t)i * K + k];
        for (int q = 0; q < a.J; ++q) {
          double acc = 0.0;
          for (int e = a.cs_ptr[q]; e < a.cs_ptr[q + 1]; ++e) {
            const int l = a.cs_idx[e];
            acc = fma(a.cs_val[e], dot(w, l < NB ? kept + (size_t)l * K : x + (size_t)(l - NB) * K), acc);
          }
          ok = ok && acc >= a.Cc[q];
        }
      }
    }
    return __all(ok ? 1 : 0) != 0;
  };
  // r(x): the log-likelihood of the observed new cells over the fit; the same bits in every lane
  auto ratio = [&](const double* x) -> double {
    double sum = 0.0;
    const int ncell = H * nr;
    for (int e = lane; e < ncell; e += WAVE) {
      const int h = e / nr, i = rows[e - h * nr];
      double w[K];
#pragma unroll
      for (int k = 0; k < K; ++k) w[k] = W[(size_t)i * K + k];
      const double eta = dot(w, x + (size_t)h * K);
      const size_t o = col + (size_t)h * N + i;
      const double cn = a.cnt[o];
      double term = 0.0;
      if (cn > 0.0) {
        if constexpr (GG) term = gg_term(a.S1[o], a.L[o], cn, eta, tab, a.G, a.lsp, ltab, etab);
        else term = poisson_term<LINK>(a.S1[o], cn, eta, ltab, lf);
      }
      sum += term + eta * fma(0.5 * a.fa[o], eta, -a.fb[o]);
    }
    return wave_sum(sum);
  };

  double* __restrict__ Vo = a.V + chain * n;
  double* __restrict__ To = a.Tau2 + chain * nR;
  const int fail_id = (int)(sg * (unsigned long long)a.M + (unsigned)j);
  double ll = feasible(m.xv) ? ratio(m.xv) : __builtin_nan("");
  if (!(fabs(ll) < INFINITY)) {                // (false for nan too)
    slice_bad_start(lane, n, nR, Vo, To, a.rounds + chain, a.unfinished + chain, a.status, fail_id);
    return;
  }
  int nrounds = 0, nunf = 0;
  bool ok = true;
  for (int sw = 0; sw < a.sweeps; ++sw) {
    const double* ds = dr ? dr + (size_t)4 * nR + (size_t)sw * per : nullptr;
    if (sw == 0 || !fixed) {
      prior_band(m, lane, nR, H * D1, lam2, a.st_ptr, a.st_row, a.st_coef);
      fill_band<K>(m, lane, n, bw, D1);
      rhs_minus_offsets<K>(m, lane, n, nR, D1, a.rcol0, a.rcoef);
      __syncthreads();
      // ---- Q = L L', rm = L^-1 rhs, then m = L^-T rm
      ok = banded_factor_forward(m.B, m.rm, m.invd, m.ptab, n, bw);
      if (!ok) break;
      __syncthreads();
      banded_backward(m.B, m.rm, m.invd, n, bw);
    }
    sweep_normals(m, lane, n, nR, ds, a.seed, stream, sw + 1);
    __syncthreads();
    banded_backward(m.B, m.ru, m.invd, n, bw);                   // nu = L^-T z
    __syncthreads();
    slice_sweep(m, lane, n, a.max_rounds, ds ? ds + n : nullptr, a.seed, stream, sw + 1, nR + n, ll, nrounds, nunf, feasible, ratio);
    if (fixed) continue;
    levels_update<K, true>(m, lane, m.xv, m.off, nR, H, D1, a.rcol0, a.rcoef, ds, (size_t)n + 1 + a.max_rounds, lam2, a.lo, a.hi, a.seed,
                     stream, sw + 1);
    __syncthreads();
  }
  slice_finish(m, lane, n, nR, ok, Vo, To, a.rounds + chain, nrounds, a.unfinished + chain, nunf, a.status, fail_id);
}

}  // namespace btf
#endif  // BTF_SLICE_FOLD_DEPTH_UNIT
