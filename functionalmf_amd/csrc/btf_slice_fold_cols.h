// Folding new columns into a slice-sampled fit  (counted under BTF_K_CRITERIA)
//
// A column of the slice-sampled models has no closed-form draw.  Given a kept sample's W_s and lam2_s the new column's curve
// v (T x K, depth-major: index t K + k) and its horseshoe+ levels form a small chain, as in btf_fold_in_cols.h, with the
// curve updated by elliptical slice sampling on an ellipse CENTRED on a Gaussian fit of the likelihood (what the reference
// does for a constrained column with ep_approx, factor.py:771-793, :891):
//     fit      per cell a_it = 1 / Sigma_fit^2 and a_it Mu_fit (0: the cell carries no fit);  A_t = sum_i a_it w_i w_i',
//              b_t = sum_i a_it Mu_it w_i;  Q = blockdiag_t(A_t) + Delta' diag(1 / (lam2 tau2)) Delta (x) I_K,  m = Q^-1 b
//     sweep    Q = L L', nu = L^-T z;  hh = r(v) + log u_h, phi = 2 pi u_a, bracket [phi - 2 pi, phi];  propose
//              v' = m + (v - m) cos phi + nu sin phi, accept when v' is feasible and r(v') >= hh, else shrink the bracket
//              towards 0 (elliptical_slice.py:59-124); after max_rounds proposals the sweep keeps v and is counted
//              r(v) = loglik(v) + sum_cells eta (a eta / 2 - a Mu),  eta_it = w_i . v_t     (the likelihood over the fit)
//              feasible: sum_t A[q,t] (w_i . v_t) >= C[q] for EVERY fitted row i and constraint q (factor.py:847-854)
//     levels   as fold_cols_kernel (factor.py:136-141); skipped when tau2 is given (held fixed)
// functionalmf_amd/slice_fold_in_cols.py restates the chain in numpy; that module is the definition.
//
// ONE launch, slice_fold_cols_kernel<K, LINK>, ONE geometry (fold_cols_kernel's): a workgroup of one wave owns the chain of
// (sample s, new column c) for all its sweeps; S * C chains in a launch.
//   fit accumulation   once per chain: for every depth the lanes walk the N rows (lane l takes rows l, l + 64, ... in
//       ascending order; the statistics lie [column][depth][row]: coalesced), the 64 partial sums are added by the xor
//       butterfly - a fixed order that depends on N alone.  A cell without a fit adds exact zeros.  A_t, b_t stay in LDS.
//   band, draw         as fold_cols_kernel: the band of Q in LDS (half bandwidth (tf + 1) K), banded_factor_forward /
//       banded_backward of btf_kernels.h in natural order.  With tau2 fixed Q is factored once.  A non-positive pivot sets
//       the chain's outputs to nan and raises status[2] with the smallest failing (global sample) * C + column in status[3].
//   feasibility        lanes over the N fitted rows, Constraints_A by its CSR non-zeros, a wave vote; tested first: an
//       infeasible proposal costs no likelihood pass.  W_s is read from global memory (it stays in L2).
//   likelihood and fit lanes over (depth, listed row): the host passes, per column, the ascending list of rows that have any
//       observed or fitted cell (a new drug is observed on few rows; an all-missing row adds nothing either way);
//       poisson_term<LINK> / gg_term on the LDS tables, staged before the first barrier; wave_sum: the same bits in every lane.
//   levels             lane = penalty row, gamma_mt.
//   bad start          infeasible, or a non-finite r: nan for that chain, status[0], and the smallest failing index in
//       status[1]; the chain does not run.
// Generator: Philox keyed (seed, stream = global sample index << 32 | column, counter = slot << 44 | element << 12 | block),
// slot 0 the start and slot r + 1 sweep r; element = penalty row for the level draws, nD + coordinate for the normals,
// nD + T K + position for u_h, u_a and the shrink uniforms - never a thread or block index: the result does not depend on
// the grid, on how S is split over calls (sample0), on how many columns a call holds or on where the states come from.
// `draws` (one flat block per chain, the layout of slice_fold_in_cols.chain) replaces every variate.
// LDS per workgroup: scols_lds_bytes; beyond SCOLS_LDS_LIMIT the call is refused - there is no second code path.
// fp64 throughout, no floating-point atomics, no spin-waits, no communication between workgroups.
#pragma once
#include "btf_device.h"
#include "btf_gamma_grid.h"

namespace btf {

constexpr size_t SCOLS_LDS_LIMIT = 156 * 1024;      // what one workgroup may hold of a CU's 160 KiB
constexpr size_t SCOLS_STATIC_LDS = 2 * LOGTAB_N * sizeof(double2) + GG_MAXG * sizeof(GgComp);   // the tables (gamma grid: all three)
constexpr double SCOLS_TAU2_START_CLIP = 9.0;       // _init_Tau2

struct SliceFoldColsArgs {
  const double* W;          // [S][N][K]
  const double* lam2;       // lam2 of sample s at lam2[s * lstride]
  const double* start; long long st_s, st_c;   // start of chain (s, c) at start[s * st_s + c * st_c + t K + k]
  const double* S1; const double* cnt; const double* L;    // [C][T][N]; L: gamma grid only
  const double* fa; const double* fb;          // [C][T][N] the fit: a = 1 / Sigma^2, a Mu (0, 0: no fit)
  const int* rptr; const int* ridx;            // [C + 1], rows of column c with an observed or fitted cell, ascending
  const int* cs_ptr; const int* cs_idx; const double* cs_val; const double* Cc; int J;    // curve constraints, CSR over [J][T]
  const double* tau2;       // [S][C][nD] local scales held fixed, or null: sampled
  const double* draws;      // [S][C][4 nD + sweeps (T K + 1 + max_rounds + 4 nD)] or null: the device generator
  const int* rcol0;         // [nD] first depth a penalty row touches
  const double* rcoef;      // [nD][tf + 2] its coefficients from there on (0 past the row's end)
  const int* st_ptr;        // [T (tf + 2) + 1] CSR of the Delta' Delta stencil per (t, d): entry (t + d, t) of the prior band
  const int* st_row;
  const double* st_coef;
  const GgComp* gg; int G; double lsp;         // gamma grid: the component table
  int fam; double par;                         // ESS_LINK_GENERIC: the family and its parameter
  double* V;                // [S][C][T][K]
  double* Tau2;             // [S][C][nD]
  int* rounds; int* unfinished;                // [S][C]
  int* status;              // [0]: 1 after a bad start, [1]: its smallest (sample0 + s) * C + c; [2], [3]: the same for a pivot
  unsigned long long seed;
  long long sample0;        // global index of sample 0 of this call (generator keys)
  double lo, hi;            // clip: stability, 1 / stability
  int lstride;
  int S, C, N, T, tf, nD, sweeps, max_rounds;
};

// the same count in slice_fold_in_cols.lds_bytes (dynamic part + the static tables)
inline size_t scols_dyn_lds_bytes(int T, int K, int tf, int nD) {
  const size_t n = (size_t)T * K, bw = (size_t)(tf + 1) * K, npairs = bw * (bw + 1) / 2;
  return 8 * (n * (bw + 1) + 6 * n + (size_t)T * tri(K) + 5 * (size_t)nD + (size_t)T * (tf + 2)) + 8 * ((npairs + 3) / 4);
}
inline size_t scols_lds_bytes(int T, int K, int tf, int nD) { return scols_dyn_lds_bytes(T, K, tf, nD) + SCOLS_STATIC_LDS; }

// the kernels live in btf_slice_fold_cols.hip (a compilation unit of their own); the C-ABI unit launches them through these
using SliceFoldColsKernel = void (*)(SliceFoldColsArgs);
using SliceFoldColsMeanKernel = void (*)(const double*, int, int, int, double*);
SliceFoldColsKernel slice_fold_cols_fn(int K, int family);     // null outside K = 1..10, family = 0..5 (ESS_FAM_*)
SliceFoldColsMeanKernel slice_fold_cols_mean_fn();

}  // namespace btf

#ifdef BTF_SLICE_FOLD_COLS_UNIT
namespace btf {

// out[s][e] = (sum_j V[s][j][e]) / M over the M fitted columns, added in ascending order; e = t K + k < TK
static __global__ void slice_fold_cols_mean_kernel(const double* __restrict__ V, int S, int M, int TK, double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)S * TK) return;
  const long long s = e / TK;
  const int r = (int)(e - s * TK);
  double sum = 0.0;
  for (int j = 0; j < M; ++j) sum += V[((size_t)s * M + j) * TK + r];
  out[e] = sum / (double)M;
}

// the generator of one element of one slot of the chain `stream` (foldc_rng of btf_fold_in_cols.h)
__device__ __forceinline__ CellRng scols_rng(unsigned long long seed, unsigned long long stream, int slot, int element) {
  CellRng g(seed, stream);
  g.ctr = ((unsigned long long)slot << 44) | ((unsigned long long)(unsigned)element << 12);
  return g;
}

template <int K, int LINK>
__global__ __launch_bounds__(WAVE) void slice_fold_cols_kernel(SliceFoldColsArgs a) {
  constexpr bool GG = LINK == ESS_LINK_GAMMA_GRID;
  constexpr int KK = tri(K), NA = KK + K;
  extern __shared__ double lds[];
  __shared__ double2 ltab[LINK == ESS_LINK_GENERIC ? 1 : LOGTAB_N];
  __shared__ double2 etab[GG ? LOGTAB_N : 1];
  __shared__ GgComp tab[GG ? GG_MAXG : 1];
  if constexpr (GG) gg_stage(GgTab{nullptr, a.gg, a.G, a.lsp}, tab, ltab, etab);
  else if constexpr (LINK == ESS_LINK_IDENTITY) log_table_build(ltab);
  else if constexpr (LINK == ESS_LINK_LOG) exp_table_build(ltab);
  const int lane = threadIdx.x;
  const int T = a.T, N = a.N, nD = a.nD, D1 = a.tf + 2, n = T * K, bw = (a.tf + 1) * K, R1 = bw + 1;
  const int s = blockIdx.x / a.C, c = blockIdx.x - s * a.C;
  double* B = lds;                      // [n][R1] the band of Q, then of L
  double* xv = B + (size_t)n * R1;      // [n] v, the state
  double* rm = xv + n;                  // [n] b -> L^-1 b -> m
  double* ru = rm + n;                  // [n] z -> nu = L^-T z
  double* xp = ru + n;                  // [n] v', the proposal
  double* bv = xp + n;                  // [n] b
  double* invd = bv + n;                // [n] 1 / L_ii
  double* A = invd + n;                 // [T][KK] packed lower triangles of A_t
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
  const int per = n + 1 + a.max_rounds + 4 * nD;                      // one sweep's record
  const size_t LD = (size_t)4 * nD + (size_t)a.sweeps * per;
  const double* dr = a.draws ? a.draws + chain * LD : nullptr;
  const double lam2 = a.lam2[(size_t)s * a.lstride];
  const double lo = a.lo, hi = a.hi;
  const bool fixed = a.tau2 != nullptr;
  const LikFam lf{a.fam, a.par};
  auto clip = [&](double x) { return fmin(fmax(x, lo), hi); };
  const double* __restrict__ W = a.W + (size_t)s * N * K;
  const size_t col = (size_t)c * T * N;                                // this column's statistics
  const int* __restrict__ rows = a.ridx + a.rptr[c];
  const int nr = a.rptr[c + 1] - a.rptr[c];

  fill_pair_table(ptab, bw);
  // ---- A_t and b_t of the fit, lanes along rows, every depth in turn (the Gaussian accumulation of fold_cols_kernel)
  for (int t = 0; t < T; ++t) {
    const double* __restrict__ fa = a.fa + col + (size_t)t * N;
    const double* __restrict__ fb = a.fb + col + (size_t)t * N;
    double acc[NA];
#pragma unroll
    for (int e = 0; e < NA; ++e) acc[e] = 0.0;
    for (int i = lane; i < N; i += WAVE) {
      double w[K];
#pragma unroll
      for (int k = 0; k < K; ++k) w[k] = W[(size_t)i * K + k];
      const double cw = fa[i], y = fb[i];
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
      for (int e = 0; e < KK; ++e) A[(size_t)t * KK + e] = acc[e];
#pragma unroll
      for (int k = 0; k < K; ++k) bv[t * K + k] = acc[KK + k];
    }
  }
  // ---- the start: the levels (sample_horseshoe_plus, Tau2 clipped as _init_Tau2 does; or the fixed scales) and v
  for (int r = lane; r < nD; r += WAVE) {
    if (fixed) { tau[r] = a.tau2[chain * nD + r]; la[r] = lb[r] = lc[r] = 1.0; continue; }
    double g0[4];
    if (dr) {
#pragma unroll
      for (int j = 0; j < 4; ++j) g0[j] = dr[(size_t)j * nD + r];
    } else {
      CellRng g = scols_rng(a.seed, stream, 0, r);
#pragma unroll
      for (int j = 0; j < 4; ++j) g0[j] = gamma_mt(0.5, g);
    }
    const double av = 1.0 / g0[0], bq = 1.0 / (av * g0[1]), cv = 1.0 / (bq * g0[2]);
    la[r] = av; lb[r] = bq; lc[r] = cv;
    tau[r] = fmin(1.0 / (cv * g0[3]), SCOLS_TAU2_START_CLIP);
  }
  {
    const double* __restrict__ st = a.start + (size_t)s * a.st_s + (size_t)c * a.st_c;
    for (int idx = lane; idx < n; idx += WAVE) xv[idx] = st[idx];
  }
  __syncthreads();

  // eta_it = w_i . x_t for the row in registers and the curve x in LDS
  auto dot = [&](const double (&w)[K], const double* x, int t) {
    double e = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) e = fma(w[k], x[t * K + k], e);
    return e;
  };
  // every restriction holds at x (a wave vote; NaN fails every comparison)
  auto feasible = [&](const double* x) -> bool {
    bool ok = true;
    if (a.J > 0) {
      for (int i = lane; i < N; i += WAVE) {
        double w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = W[(size_t)i * K + k];
        for (int q = 0; q < a.J; ++q) {
          double acc = 0.0;
          for (int e = a.cs_ptr[q]; e < a.cs_ptr[q + 1]; ++e) acc = fma(a.cs_val[e], dot(w, x, a.cs_idx[e]), acc);
          ok = ok && acc >= a.Cc[q];
        }
      }
    }
    return __all(ok ? 1 : 0) != 0;
  };
  // r(x): the log-likelihood of the observed cells over the fit; the same bits in every lane
  auto ratio = [&](const double* x) -> double {
    double sum = 0.0;
    const int ncell = T * nr;
    for (int e = lane; e < ncell; e += WAVE) {
      const int t = e / nr, i = rows[e - t * nr];
      double w[K];
#pragma unroll
      for (int k = 0; k < K; ++k) w[k] = W[(size_t)i * K + k];
      const double eta = dot(w, x, t);
      const size_t off = col + (size_t)t * N + i;
      const double cn = a.cnt[off];
      double term = 0.0;
      if (cn > 0.0) {
        if constexpr (GG) term = gg_term(a.S1[off], a.L[off], cn, eta, tab, a.G, a.lsp, ltab, etab);
        else term = poisson_term<LINK>(a.S1[off], cn, eta, ltab, lf);
      }
      sum += term + eta * fma(0.5 * a.fa[off], eta, -a.fb[off]);
    }
    return wave_sum(sum);
  };
  // number `pos` of the uniforms of sweep `sw` (0: u_h, 1: u_a, 2 + rd: the shrink uniforms)
  auto uniform = [&](int sw, int pos) {
    if (dr) return dr[(size_t)4 * nD + (size_t)sw * per + n + pos];
    CellRng g = scols_rng(a.seed, stream, sw + 1, nD + n + pos);
    return g.uniform();
  };

  const double bad = __builtin_nan("");
  double* __restrict__ Vo = a.V + chain * n;
  double* __restrict__ To = a.Tau2 + chain * nD;
  const int fail_id = (int)(sg * (unsigned long long)a.C + (unsigned)c);
  double ll = feasible(xv) ? ratio(xv) : bad;
  if (!(fabs(ll) < INFINITY)) {                // (false for nan too)
    for (int idx = lane; idx < n; idx += WAVE) Vo[idx] = bad;
    for (int r = lane; r < nD; r += WAVE) To[r] = bad;
    if (lane == 0) {
      a.rounds[chain] = 0; a.unfinished[chain] = 0;
      a.status[0] = 1;
      atomicMin(&a.status[1], fail_id);
    }
    return;
  }
  const double two_pi = 6.283185307179586476925286766559;
  int nrounds = 0, nunf = 0;
  bool ok = true;
  for (int sw = 0; sw < a.sweeps; ++sw) {
    const double* ds = dr ? dr + (size_t)4 * nD + (size_t)sw * per : nullptr;
    if (sw == 0 || !fixed) {
      // ---- the prior band from 1 / (lam2 tau2), then the band of Q: column nn = t K + k holds the entries (nn + off, nn)
      for (int r = lane; r < nD; r += WAVE) itau[r] = 1.0 / (lam2 * tau[r]);
      __syncthreads();
      for (int e0 = lane; e0 < T * D1; e0 += WAVE) {
        double sum = 0.0;
        for (int e = a.st_ptr[e0]; e < a.st_ptr[e0 + 1]; ++e) sum = fma(a.st_coef[e], itau[a.st_row[e]], sum);
        pb[e0] = sum;
      }
      __syncthreads();
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
      for (int idx = lane; idx < n; idx += WAVE) rm[idx] = bv[idx];
      __syncthreads();
      // ---- Q = L L', rm = L^-1 b, then m = L^-T rm
      ok = banded_factor_forward(B, rm, invd, ptab, n, bw);
      if (!ok) break;
      __syncthreads();
      banded_backward(B, rm, invd, n, bw);
    }
    for (int idx = lane; idx < n; idx += WAVE) {
      double z;
      if (ds) z = ds[idx];
      else { CellRng g = scols_rng(a.seed, stream, sw + 1, nD + idx); z = g.normal(); }
      ru[idx] = z;
    }
    __syncthreads();
    banded_backward(B, ru, invd, n, bw);                   // nu = L^-T z
    __syncthreads();
    // ---- the slice: shrink the bracket until a feasible proposal lies on it
    const double hh = ll + log(uniform(sw, 0));
    double phi = two_pi * uniform(sw, 1);
    double blo = phi - two_pi, bhi = phi;
    bool accepted = false;
    for (int rd = 0; rd < a.max_rounds; ++rd) {
      double sn, cs;
      sincos(phi, &sn, &cs);
      for (int idx = lane; idx < n; idx += WAVE) xp[idx] = rm[idx] + fma(xv[idx] - rm[idx], cs, ru[idx] * sn);
      __syncthreads();
      if (feasible(xp)) {
        ++nrounds;
        const double llp = ratio(xp);
        if (llp >= hh) {
          for (int idx = lane; idx < n; idx += WAVE) xv[idx] = xp[idx];
          ll = llp;
          accepted = true;
          break;
        }
      }
      if (phi > 0.0) bhi = phi; else blo = phi;
      if (rd + 1 < a.max_rounds) phi = fma(bhi - blo, uniform(sw, 2 + rd), blo);
      __syncthreads();                                     // (every lane has read xp before the next proposal overwrites it)
    }
    if (!accepted) ++nunf;                                 // the cap: the sweep keeps v
    __syncthreads();
    if (fixed) continue;
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
        for (int k = 0; k < K; ++k) dv[k] = fma(cf, xv[t * K + k], dv[k]);
      }
      double dsq = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) dsq = fma(dv[k], dv[k], dsq);
      double g4[4];
      if (ds) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g4[j] = ds[(size_t)n + 1 + a.max_rounds + (size_t)j * nD + r];
      } else {
        CellRng g = scols_rng(a.seed, stream, sw + 1, r);
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
  for (int idx = lane; idx < n; idx += WAVE) Vo[idx] = ok ? xv[idx] : bad;
  for (int r = lane; r < nD; r += WAVE) To[r] = ok ? tau[r] : bad;
  if (lane == 0) {
    a.rounds[chain] = nrounds;
    a.unfinished[chain] = nunf;
    if (!ok) {
      a.status[2] = 1;
      atomicMin(&a.status[3], fail_id);
    }
  }
}

}  // namespace btf
#endif  // BTF_SLICE_FOLD_COLS_UNIT
