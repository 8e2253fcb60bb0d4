// The chain core of the column and depth fold-in kernels  (no kernel of its own)
//
// fold_cols_kernel (btf_fold_in_cols.h), fold_depth_kernel (btf_fold_in_depth.h), slice_fold_cols_kernel
// (btf_slice_fold_cols.h) and slice_fold_depth_kernel (btf_slice_fold_depth.h) each run, in a workgroup of ONE wave, the
// chain of a curve v (T x K, depth-major: index t K + k; the depth kernels: the H new depths) and the horseshoe+ levels
// (tau2, c, b, a) of its nD penalty rows.  The steps the four share exist here once; every step takes LDS pointers, the
// lane and sizes - never the argument block of one kernel.
//   generator      chain_rng: Philox keyed (seed, stream = global sample index << 32 | column, counter = slot << 44 |
//       element << 12 | block), slot 0 the start and slot r + 1 sweep r; element = penalty row for the level draws,
//       nD + coordinate for the normals, nD + T K + position for the uniforms of a slice sweep - never a thread or block index.
//       `draws` (one flat block per chain: 4 nD start gammas, then per sweep T K normals, [1 + max_rounds uniforms,] 4 nD
//       gammas) replaces every variate.
//   accumulation   accumulate_blocks: for every depth the lanes walk the N rows (lane l takes rows l, l + 64, ... in
//       ascending order; the statistics lie [column][depth][row]: one coalesced load per 64 rows), keep the K (K + 1) / 2 + K
//       running sums of their rows in registers, and the 64 partial sums are added by the xor butterfly - a fixed order
//       that depends on N alone.  A cell without weight adds exact zeros.  A_t and b_t stay in LDS.
//   negbin         negbin_draw_depth, negbin_accumulate: the Negative-Binomial family's weights omega ~ PG(ysum + c r, w . v)
//       of one depth drawn into LDS in a pass of their own, then accumulate_depth with kappa = (ysum - c r) / 2.
//   band           prior_band, fill_band: the band of Q in LDS, column nn at B[nn (bw + 1)]; within a depth the offsets reach
//       K - 1, across depths the prior couples (t, k) with (t + d, k), d <= tf + 1, at offset d K.  The prior band is
//       formed from 1 / (lam2 tau2) through the CSR of the Delta' Delta stencil as band_side (btf_kernels.h) does.
//   offsets        tail_offsets, rhs_minus_offsets (the depth kernels): off = D_o V_s[j] from the kept tail in LDS, and
//       rhs = b - D_n' diag(1 / (lam2 tau2)) off with the rows of R added in ascending order.
//   levels         levels_start, levels_update: lane = penalty row, gamma_mt (btf_kernels.h) on a generator of the row.
//   slice          slice_sweep: one elliptical slice update about the centre m; what is feasible and the likelihood
//       ratio are the caller's.
//   epilogues      gibbs_finish (status[0], [1]: a non-positive pivot), slice_bad_start (status[0], [1]) and slice_finish
//       (status[2], [3]): nan for the chain, the flag, and the smallest failing index by integer atomicMin.
// LDS: FoldChainLds names the arrays of a chain, fold_chain_layout carves them and counts them - the kernels' pointers, the
// byte counts the host refuses by and the launch size are this one description.  Beyond FOLD_CHAIN_LDS_LIMIT a call is
// refused - there is no second code path.  fp64 throughout, no floating-point atomics.
#pragma once
#include "btf_device.h"
#include <math.h>

namespace btf {

constexpr size_t FOLD_CHAIN_LDS_LIMIT = 156 * 1024;      // what one workgroup may hold of a CU's 160 KiB beside its static tables
constexpr int FOLD_CHAIN_MAX_TRIALS = 32;                // PG_AUTO_EXACT_MAX: the counts drawn exactly (btf_fold_in.h)
constexpr unsigned long long FOLD_CHAIN_PG_SLOT = 0xFFFFFULL;   // the generator slot of the Polya-Gamma key: sweeps stay below it
constexpr double FOLD_CHAIN_TAU2_START_CLIP = 9.0;       // _init_Tau2

// half bandwidth of the H K-wide system of the depth kernels: for H <= tf + 1 it is narrower than the band of the prior
__host__ __device__ constexpr int fold_depth_bandwidth(int H, int K, int tf) { return (tf + 1) * K < H * K - 1 ? (tf + 1) * K : H * K - 1; }

// the LDS of one chain; n = T K.  xv and xp: the slice kernels; off and vt: the depth kernels (null otherwise).
struct FoldChainLds {
  double* B;                // [n][bw + 1] the band of Q, then of L
  double* xv;               // [n] v, the state of a slice chain
  double* rm;               // [n] rhs -> L^-1 rhs -> mean
  double* ru;               // [n] z -> L^-T z (the Gibbs kernels: -> v)
  double* xp;               // [n] v', the proposal of a slice chain
  double* invd;             // [n] 1 / L_ii
  double* bv;               // [n] b
  double* A;                // [T][K (K + 1) / 2] packed lower triangles of A_t
  double *tau, *lc, *lb, *la;   // [nD] x 4: tau2, c, b, a
  double* itau;             // [nD] 1 / (lam2 tau2)
  double* off;              // [nD][K] D_o V_s[j]
  double* pb;               // [T][tf + 2] the prior band: entry (t + d, t)
  double* vt;               // [L][K] the kept tail
  double* om;               // [nom] the Polya-Gamma weights of one depth, nom = N (the Negative-Binomial family; null otherwise)
  unsigned short* ptab;     // [bw (bw + 1) / 2] the pair table of banded_factor_forward
};

// Carves the arrays of a chain of T depths with nD penalty rows and half bandwidth bw out of `base` and returns the bytes
// they take; a null base only counts.  L: the kept depths of a depth kernel's tail, 0 for a column kernel.  nom: the rows of
// the Negative-Binomial family's weight buffer, 0 for every other family.
__host__ __device__ inline size_t fold_chain_layout(FoldChainLds& m, double* base, int T, int K, int tf, int bw, int nD, int L, bool slice,
                                                    int nom = 0) {
  const size_t n = (size_t)T * K, npairs = (size_t)bw * (bw + 1) / 2;
  size_t used = 0;
  auto take = [&](size_t count) {
    double* p = base ? base + used : nullptr;
    used += count;
    return p;
  };
  m.B = take(n * (bw + 1));
  m.xv = slice ? take(n) : nullptr;
  m.rm = take(n); m.ru = take(n);
  m.xp = slice ? take(n) : nullptr;
  m.invd = take(n); m.bv = take(n);
  m.A = take((size_t)T * tri(K));
  m.tau = take(nD); m.lc = take(nD); m.lb = take(nD); m.la = take(nD); m.itau = take(nD);
  m.off = L > 0 ? take((size_t)nD * K) : nullptr;
  m.pb = take((size_t)T * (tf + 2));
  m.vt = L > 0 ? take((size_t)L * K) : nullptr;
  m.om = nom > 0 ? take((size_t)nom) : nullptr;
  m.ptab = reinterpret_cast<unsigned short*>(take((npairs + 3) / 4));
  return 8 * used;
}
inline size_t fold_chain_lds_bytes(int T, int K, int tf, int bw, int nD, int L, bool slice, int nom = 0) {
  FoldChainLds m;
  return fold_chain_layout(m, nullptr, T, K, tf, bw, nD, L, slice, nom);
}

}  // namespace btf

#if defined(BTF_FOLD_COLS_UNIT) || defined(BTF_FOLD_DEPTH_UNIT) || defined(BTF_SLICE_FOLD_COLS_UNIT) || defined(BTF_SLICE_FOLD_DEPTH_UNIT)
#include "btf_kernels.h"        // banded_factor_forward / banded_backward, fill_pair_table, CellRng, gamma_mt

namespace btf {

// the generator of one element of one slot of the chain `stream`
__device__ __forceinline__ CellRng chain_rng(unsigned long long seed, unsigned long long stream, int slot, int element) {
  CellRng g(seed, stream);
  g.ctr = ((unsigned long long)slot << 44) | ((unsigned long long)(unsigned)element << 12);
  return g;
}

// the right-hand side of a cell is its ys
struct CellSum {
  __device__ __forceinline__ double operator()(int, int, double, double ys) const { return ys; }
};

// A_t = scale sum_i weight_it w_i w_i' and b_t = scale sum_i rhs_it w_i at ONE depth t, lanes along rows; cn and ys: the [N]
// statistics of the depth.  row_weight(t, i, w, cn_it) gives the weight of a row and row_rhs(t, i, cn_it, ys_it) its
// right-hand side (CellSum: ys_it itself): every lane of the wave calls them in every block of 64 rows (a lane past N with
// row N - 1 and cn = ys = 0: its cell then adds exact zeros, which leave every running sum as it is up to the sign of a
// zero), so they may hold wave-wide steps.
template <int K, class RowWeight, class RowRhs = CellSum>
__device__ __forceinline__ void accumulate_depth(double* A, double* bv, int lane, const double* __restrict__ W,
                                                 const double* __restrict__ cn, const double* __restrict__ ys, int t, int N,
                                                 double scale, RowWeight row_weight, RowRhs row_rhs = RowRhs()) {
  constexpr int KK = tri(K), NA = KK + K;
  double acc[NA];
#pragma unroll
  for (int e = 0; e < NA; ++e) acc[e] = 0.0;
  for (int i0 = 0; i0 < N; i0 += WAVE) {
    const int i = i0 + lane;
    const bool row_ok = i < N;
    const int ic = row_ok ? i : N - 1;
    double w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = W[(size_t)ic * K + k];
    const double cv = row_ok ? cn[ic] : 0.0;
    const double cw = row_weight(t, ic, w, cv);
    const double y = row_rhs(t, ic, cv, row_ok ? ys[ic] : 0.0);
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
    for (int e = 0; e < KK; ++e) A[(size_t)t * KK + e] = acc[e] * scale;
#pragma unroll
    for (int k = 0; k < K; ++k) bv[t * K + k] = acc[KK + k] * scale;
  }
}
// the same for every depth t < T in turn; cn and ys: [T][N]
template <int K, class RowWeight>
__device__ __forceinline__ void accumulate_blocks(double* A, double* bv, int lane, const double* __restrict__ W, const double* cn0,
                                                  const double* ys0, int T, int N, double scale, RowWeight row_weight) {
  for (int t = 0; t < T; ++t) accumulate_depth<K>(A, bv, lane, W, cn0 + (size_t)t * N, ys0 + (size_t)t * N, t, N, scale, row_weight);
}
// the weight of a row is its cn
struct CellWeight {
  template <int K>
  __device__ __forceinline__ double operator()(int, int, const double (&)[K], double cn) const { return cn; }
};

// The Negative-Binomial family (factor.py:506-511, 553): a cell with c observed replicates, their sum ysum and the rate r of
// its (sample, chain, row, depth) is the Binomial cell with pseudo-data b = ysum + c r, kappa = (ysum - c r) / 2.
struct NegbinRate {
  const double* rate;       // the rate of (row i, depth t) of this chain at rate[i row + t depth]: the sample's and the chain's
  long long row, depth;     //   strides are folded into the pointer; 0 on an axis the rate is shared along
  const double* omega;      // [T][N] the weights of this chain's sweep in the place of every draw, or null
};
// omega_it ~ PG(ysum_it + c_it r_it, w_i . v_t) from the current v for ONE depth, left in m.om ([N], lane l its rows l,
// l + 64, ...): the draws have a pass of their own so that the series sampler's second generator and candidate loop never
// meet the K (K + 1) / 2 + K running sums of accumulate_depth in the register file.  The sampler is the one the
// Negative-Binomial sweeps draw count data with (pg_draw_series below PG_NORMAL_B, pg_draw_normal from there on) on a CellRng
// keyed (pg_key, (sweep T + t) N + i) - the key of the Binomial family's cells, never a thread or block index.  c = 0: weight
// 0 without a draw.  A psi that is not finite (or beyond 1e8, where the series' term count leaves an int) gives nan: the
// factorisation then fails and the chain is flagged.
template <int K>
__device__ __forceinline__ void negbin_draw_depth(const FoldChainLds& m, int lane, const double* __restrict__ W,
                                                  const double* __restrict__ cn, const double* __restrict__ ys, const double* v, int t,
                                                  int T, int N, const NegbinRate& nb, unsigned long long pg_key, int sw) {
  for (int i = lane; i < N; i += WAVE) {
    const double c = cn[i];
    double om = 0.0;
    if (c > 0.0) {
      if (nb.omega) om = nb.omega[(size_t)t * N + i];
      else {
        double psi = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) psi = fma(W[(size_t)i * K + k], v[t * K + k], psi);
        const double b = ys[i] + c * nb.rate[i * nb.row + t * nb.depth];
        if (!(fabs(psi) <= 1e8)) om = __builtin_nan("");
        else {
          CellRng g(pg_key, ((unsigned long long)sw * T + t) * N + i);
          om = b >= (double)PG_NORMAL_B ? pg_draw_normal(b, psi, g) : pg_draw_series(b, psi, g);
        }
      }
    }
    m.om[i] = om;
  }
}
// A_t = sum_i omega_it w_i w_i' and b_t = sum_i kappa_it w_i for every depth: the draw pass, then the accumulation reading it
template <int K>
__device__ __forceinline__ void negbin_accumulate(const FoldChainLds& m, int lane, const double* __restrict__ W, const double* cn0,
                                                  const double* ys0, const double* v, int T, int N, const NegbinRate& nb,
                                                  unsigned long long pg_key, int sw) {
  for (int t = 0; t < T; ++t) {
    const double* cn = cn0 + (size_t)t * N;
    const double* ys = ys0 + (size_t)t * N;
    negbin_draw_depth<K>(m, lane, W, cn, ys, v, t, T, N, nb, pg_key, sw);
    __syncthreads();
    accumulate_depth<K>(
        m.A, m.bv, lane, W, cn, ys, t, N, 1.0, [&](int, int i, const double (&)[K], double c) { return c > 0.0 ? m.om[i] : 0.0; },
        [&](int tt, int i, double c, double y) { return c > 0.0 ? 0.5 * (y - c * nb.rate[i * nb.row + tt * nb.depth]) : 0.0; });
    __syncthreads();
  }
}

// the start of the levels: sample_horseshoe_plus with Tau2 clipped as _init_Tau2 does, from the 4 nD gammas at `dr` or the
// generator's slot 0; or, with `fixed` (this chain's nD scales), tau2 held there and the other levels at 1
__device__ __forceinline__ void levels_start(const FoldChainLds& m, int lane, int nD, const double* dr, const double* fixed,
                                             unsigned long long seed, unsigned long long stream) {
  for (int r = lane; r < nD; r += WAVE) {
    if (fixed) { m.tau[r] = fixed[r]; m.la[r] = m.lb[r] = m.lc[r] = 1.0; continue; }
    double g0[4];
    if (dr) {
#pragma unroll
      for (int j = 0; j < 4; ++j) g0[j] = dr[(size_t)j * nD + r];
    } else {
      CellRng g = chain_rng(seed, stream, 0, r);
#pragma unroll
      for (int j = 0; j < 4; ++j) g0[j] = gamma_mt(0.5, g);
    }
    const double av = 1.0 / g0[0], bq = 1.0 / (av * g0[1]), cv = 1.0 / (bq * g0[2]);
    m.la[r] = av; m.lb[r] = bq; m.lc[r] = cv;
    m.tau[r] = fmin(1.0 / (cv * g0[3]), FOLD_CHAIN_TAU2_START_CLIP);
  }
}

// itau = 1 / (lam2 tau2), then the prior band pb[t (tf + 2) + d] = entry (t + d, t) through the CSR of the stencil; ends
// behind a barrier: pb is ready to be read
__device__ __forceinline__ void prior_band(const FoldChainLds& m, int lane, int nD, int nband, double lam2, const int* st_ptr,
                                           const int* st_row, const double* st_coef) {
  for (int r = lane; r < nD; r += WAVE) m.itau[r] = 1.0 / (lam2 * m.tau[r]);
  __syncthreads();
  for (int e0 = lane; e0 < nband; e0 += WAVE) {
    double sum = 0.0;
    for (int e = st_ptr[e0]; e < st_ptr[e0 + 1]; ++e) sum = fma(st_coef[e], m.itau[st_row[e]], sum);
    m.pb[e0] = sum;
  }
  __syncthreads();
}

// the band of Q: column nn = t K + k holds the entries (nn + off, nn), off = 0..bw (t2 - t <= tf + 1 as off <= (tf + 1) K)
template <int K>
__device__ __forceinline__ void fill_band(const FoldChainLds& m, int lane, int n, int bw, int D1) {
  constexpr int KK = tri(K);
  const int R1 = bw + 1;
  for (int idx = lane; idx < n * R1; idx += WAVE) {
    const int nn = idx / R1, off = idx - nn * R1;
    const int t = nn / K, k = nn - t * K;
    const int row = nn + off, t2 = row / K, k2 = row - t2 * K;
    double v = 0.0;
    if (row < n) {
      if (t2 == t) v = m.A[(size_t)t * KK + lidx(k2, k)];
      if (k2 == k) v += m.pb[t * D1 + (t2 - t)];
    }
    m.B[idx] = v;
  }
}

// the kept tail ([L][K] at src) into LDS, then the offsets D_o V_s[j]: row r reaches the kept depths rcol0 + e < 0, tail
// index L + rcol0 + e
template <int K>
__device__ __forceinline__ void tail_offsets(const FoldChainLds& m, int lane, const double* __restrict__ src, int L, int nR, int D1,
                                             const int* rcol0, const double* rcoef) {
  for (int idx = lane; idx < L * K; idx += WAVE) m.vt[idx] = src[idx];
  __syncthreads();
  for (int idx = lane; idx < nR * K; idx += WAVE) {
    const int r = idx / K, k = idx - r * K, t0 = rcol0[r];
    double sum = 0.0;
    for (int e = 0; e < D1; ++e) {
      const int t = t0 + e;
      if (t < 0 && L + t >= 0) sum = fma(rcoef[(size_t)r * D1 + e], m.vt[(L + t) * K + k], sum);
    }
    m.off[idx] = sum;
  }
}

// rm = b - D_n' diag(1 / (lam2 tau2)) off, the rows of R in ascending order
template <int K>
__device__ __forceinline__ void rhs_minus_offsets(const FoldChainLds& m, int lane, int n, int nR, int D1, const int* rcol0,
                                                  const double* rcoef) {
  for (int idx = lane; idx < n; idx += WAVE) {
    const int t = idx / K, k = idx - t * K;
    double sum = 0.0;
    for (int r = 0; r < nR; ++r) {
      const int e = t - rcol0[r];
      if (e >= 0 && e < D1) sum = fma(rcoef[(size_t)r * D1 + e] * m.itau[r], m.off[r * K + k], sum);
    }
    m.rm[idx] = m.bv[idx] - sum;
  }
}

// ru = the n normals of a sweep: its record `ds`, or the generator's slot `slot` at the elements behind the nD level rows.
// copy_rhs: rm = b in the same pass (a Gibbs column kernel, whose right-hand side has no offsets).
__device__ __forceinline__ void sweep_normals(const FoldChainLds& m, int lane, int n, int nD, const double* ds, unsigned long long seed,
                                              unsigned long long stream, int slot, bool copy_rhs = false) {
  for (int idx = lane; idx < n; idx += WAVE) {
    if (copy_rhs) m.rm[idx] = m.bv[idx];
    double z;
    if (ds) z = ds[idx];
    else { CellRng g = chain_rng(seed, stream, slot, nD + idx); z = g.normal(); }
    m.ru[idx] = z;
  }
}

// The levels given the curve x (factor.py:136-141), lane = penalty row: dv = off + D x with off null for the column kernels;
// the gammas of the sweep at ds[gofs ...] or from the generator's slot.  A row's window may leave the T depths of x.  SKIP
// (the depth kernels): a term before depth 0 (a kept depth, in off) or past the end is skipped.  Otherwise (the column
// kernels, whose windows start at depth >= 0): a term past the end is added at the last depth with its coefficient, which
// is 0 there - no branch in the loop.  Both give the same sum of squares: a zero term can turn a -0.0 in dv into 0.0 at most.
template <int K, bool SKIP>
__device__ __forceinline__ void levels_update(const FoldChainLds& m, int lane, const double* x, const double* off, int nD, int T, int D1, const int* rcol0,
                                              const double* rcoef, const double* ds, size_t gofs, double lam2, double lo, double hi,
                                              unsigned long long seed, unsigned long long stream, int slot) {
  auto clip = [&](double v) { return fmin(fmax(v, lo), hi); };
  for (int r = lane; r < nD; r += WAVE) {
    const int t0 = rcol0[r];
    double dv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) dv[k] = off ? off[r * K + k] : 0.0;
    for (int e = 0; e < D1; ++e) {
      if (SKIP && (t0 + e < 0 || t0 + e >= T)) continue;
      const double cf = rcoef[(size_t)r * D1 + e];
      const int t = min(t0 + e, T - 1);
#pragma unroll
      for (int k = 0; k < K; ++k) dv[k] = fma(cf, x[t * K + k], dv[k]);
    }
    double dsq = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) dsq = fma(dv[k], dv[k], dsq);
    double g4[4];
    if (ds) {
#pragma unroll
      for (int j = 0; j < 4; ++j) g4[j] = ds[gofs + (size_t)j * nD + r];
    } else {
      CellRng g = chain_rng(seed, stream, slot, r);
      g4[0] = gamma_mt(0.5 * (K + 1), g);
#pragma unroll
      for (int j = 1; j < 4; ++j) g4[j] = gamma_mt(1.0, g);
    }
    const double rate = dsq / (2.0 * lam2) + 1.0 / clip(m.lc[r]);
    const double tv = clip(rate) / g4[0];
    const double cv = clip(1.0 / tv + 1.0 / m.lb[r]) / g4[1];
    const double bq = clip(1.0 / cv + 1.0 / m.la[r]) / g4[2];
    const double av = clip(1.0 / bq + 1.0) / g4[3];
    m.tau[r] = tv; m.lc[r] = cv; m.lb[r] = bq; m.la[r] = av;
  }
}

// the last state of a Gibbs chain: v (ru), the last conditional mean (rm) and tau2; after a failed factorisation nan, the
// flag in status[0] and the smallest failing index in status[1]
__device__ __forceinline__ void gibbs_finish(const FoldChainLds& m, int lane, int n, int nD, bool ok, double* __restrict__ Vo,
                                             double* __restrict__ Mo, double* __restrict__ To, int* status, int fail_id) {
  const double bad = __builtin_nan("");
  for (int idx = lane; idx < n; idx += WAVE) { Vo[idx] = ok ? m.ru[idx] : bad; Mo[idx] = ok ? m.rm[idx] : bad; }
  for (int r = lane; r < nD; r += WAVE) To[r] = ok ? m.tau[r] : bad;
  if (!ok && lane == 0) {
    status[0] = 1;
    atomicMin(&status[1], fail_id);
  }
}

// One elliptical slice update of the state xv about the centre rm with nu = ru (elliptical_slice.py:59-124): hh = ll +
// log u_h, phi = 2 pi u_a, bracket [phi - 2 pi, phi]; propose v' = m + (v - m) cos phi + nu sin phi into xp, accept when
// feasible(xp) and ratio(xp) >= hh, else shrink the bracket towards 0.  Feasibility is tested first: an infeasible proposal
// costs no likelihood pass and is not counted in nrounds.  After max_rounds proposals the sweep keeps v and is counted in
// nunf.  The uniforms (0: u_h, 1: u_a, 2 + rd: the shrink uniforms) lie at `us` or come from the generator's elements
// uelem + position of the slot.  ll = ratio(xv) on entry and on exit; ends behind a barrier.
template <class Feasible, class Ratio>
__device__ __forceinline__ void slice_sweep(const FoldChainLds& m, int lane, int n, int max_rounds, const double* us,
                                            unsigned long long seed, unsigned long long stream, int slot, int uelem, double& ll,
                                            int& nrounds, int& nunf, Feasible feasible, Ratio ratio) {
  auto uniform = [&](int pos) {
    if (us) return us[pos];
    CellRng g = chain_rng(seed, stream, slot, uelem + pos);
    return g.uniform();
  };
  const double two_pi = 6.283185307179586476925286766559;
  const double hh = ll + log(uniform(0));
  double phi = two_pi * uniform(1);
  double blo = phi - two_pi, bhi = phi;
  bool accepted = false;
  for (int rd = 0; rd < max_rounds; ++rd) {
    double sn, cs;
    sincos(phi, &sn, &cs);
    for (int idx = lane; idx < n; idx += WAVE) m.xp[idx] = m.rm[idx] + fma(m.xv[idx] - m.rm[idx], cs, m.ru[idx] * sn);
    __syncthreads();
    if (feasible(m.xp)) {
      ++nrounds;
      const double llp = ratio(m.xp);
      if (llp >= hh) {
        for (int idx = lane; idx < n; idx += WAVE) m.xv[idx] = m.xp[idx];
        ll = llp;
        accepted = true;
        break;
      }
    }
    if (phi > 0.0) bhi = phi; else blo = phi;
    if (rd + 1 < max_rounds) phi = fma(bhi - blo, uniform(2 + rd), blo);
    __syncthreads();                                     // (every lane has read xp before the next proposal overwrites it)
  }
  if (!accepted) ++nunf;                                 // the cap: the sweep keeps v
  __syncthreads();
}

// a bad start (infeasible, or a non-finite r): nan for the chain, which does not run; status[0] and the smallest failing index in status[1]
__device__ __forceinline__ void slice_bad_start(int lane, int n, int nD, double* __restrict__ Vo, double* __restrict__ To, int* rounds,
                                                int* unfinished, int* status, int fail_id) {
  const double bad = __builtin_nan("");
  for (int idx = lane; idx < n; idx += WAVE) Vo[idx] = bad;
  for (int r = lane; r < nD; r += WAVE) To[r] = bad;
  if (lane == 0) {
    *rounds = 0; *unfinished = 0;
    status[0] = 1;
    atomicMin(&status[1], fail_id);
  }
}

// the last state of a slice chain and its counters; after a failed factorisation nan, status[2] and the smallest failing
// index in status[3]
__device__ __forceinline__ void slice_finish(const FoldChainLds& m, int lane, int n, int nD, bool ok, double* __restrict__ Vo,
                                             double* __restrict__ To, int* rounds, int nrounds, int* unfinished, int nunf, int* status,
                                             int fail_id) {
  const double bad = __builtin_nan("");
  for (int idx = lane; idx < n; idx += WAVE) Vo[idx] = ok ? m.xv[idx] : bad;
  for (int r = lane; r < nD; r += WAVE) To[r] = ok ? m.tau[r] : bad;
  if (lane == 0) {
    *rounds = nrounds;
    *unfinished = nunf;
    if (!ok) {
      status[2] = 1;
      atomicMin(&status[3], fail_id);
    }
  }
}

}  // namespace btf
#endif  // a fold-in unit
