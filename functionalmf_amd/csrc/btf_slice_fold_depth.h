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
//     levels   dv = off + D_n v, then as fold_depth_kernel; skipped when tau2 is given (held fixed)
// functionalmf_amd/slice_fold_in_depth.py restates the chain in numpy; that module is the definition.
//
// ONE launch, slice_fold_depth_kernel<K, LINK>, ONE geometry (slice_fold_cols_kernel's): a workgroup of one wave owns the
// chain of (sample s, fitted column j) for all its sweeps; S * M chains in a launch.
//   kept tail          the last Lt = max(min(T, tf + 1), B) depths of V_s[j] are read once into LDS; off follows from them.
//   fit accumulation   once per chain: for every new depth the lanes walk the N rows (lane l takes rows l, l + 64, ...; the
//       statistics lie [column][depth][row]: coalesced), the 64 partial sums are added by the xor butterfly - a fixed order
//       that depends on N alone.  A_h, b_h stay in LDS.
//   band, draw         as fold_depth_kernel: the band of the H K-wide Q in LDS (half bandwidth min((tf + 1) K, H K - 1)),
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
// instantiation uses scratch (0 bytes / lane), 106 SGPR each, AGPR 0 except 22 at K = 10:
//   log link (static LDS 2048 B)         165 163 164 167 168 170 172 193 233 256
//   identity link (2048 B)               157 155 156 159 160 162 164 193 233 256
//   generic: families 2..4 (0 B)         165 163 164 167 168 170 172 193 233 256
//   gamma grid (8192 B)                  172 169 170 173 174 176 178 193 233 256
// One-wave workgroups: a CU holds as many chains as its LDS allows (eight at 18.4 KB), so the register count does not bound
// the occupancy below K = 10.
#pragma once
#include "btf_device.h"
#include "btf_gamma_grid.h"

namespace btf {

constexpr size_t SDEPTH_LDS_LIMIT = 156 * 1024;      // what one workgroup may hold of a CU's 160 KiB
constexpr size_t SDEPTH_STATIC_LDS = 2 * LOGTAB_N * sizeof(double2) + GG_MAXG * sizeof(GgComp);   // the tables (gamma grid: all three)
constexpr double SDEPTH_TAU2_START_CLIP = 9.0;       // _init_Tau2

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

__host__ __device__ constexpr int sdepth_bandwidth(int H, int K, int tf) { return (tf + 1) * K < H * K - 1 ? (tf + 1) * K : H * K - 1; }

// the same count in slice_fold_in_depth.lds_bytes (dynamic part + the static tables): foldd_lds_bytes with six H K vectors
// (v, m, nu, v', b, the pivots) and the tail of Lt = max(min(T, tf + 1), B) kept depths
inline size_t sdepth_dyn_lds_bytes(int H, int K, int tf, int nR, int Lt) {
  const size_t n = (size_t)H * K, bw = (size_t)sdepth_bandwidth(H, K, tf), npairs = bw * (bw + 1) / 2;
  return 8 * (n * (bw + 1) + 6 * n + (size_t)H * tri(K) + 5 * (size_t)nR + (size_t)nR * K + (size_t)H * (tf + 2) + (size_t)Lt * K) +
         8 * ((npairs + 3) / 4);
}
inline size_t sdepth_lds_bytes(int H, int K, int tf, int nR, int Lt) { return sdepth_dyn_lds_bytes(H, K, tf, nR, Lt) + SDEPTH_STATIC_LDS; }

// the kernels live in btf_slice_fold_depth.hip (a compilation unit of their own); the C-ABI unit launches them through this
using SliceFoldDepthKernel = void (*)(SliceFoldDepthArgs);
SliceFoldDepthKernel slice_fold_depth_fn(int K, int family);     // null outside K = 1..10, family = 0..5 (ESS_FAM_*)

}  // namespace btf

#ifdef BTF_SLICE_FOLD_DEPTH_UNIT
namespace btf {

// the generator of one element of one slot of the chain `stream` (scols_rng of btf_slice_fold_cols.h)
__device__ __forceinline__ CellRng sdepth_rng(unsigned long long seed, unsigned long long stream, int slot, int element) {
  CellRng g(seed, stream);
  g.ctr = ((unsigned long long)slot << 44) | ((unsigned long long)(unsigned)element << 12);
  return g;
}

template <int K, int LINK>
__global__ __launch_bounds__(WAVE) void slice_fold_depth_kernel(SliceFoldDepthArgs a) {
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
  const int H = a.H, N = a.N, nR = a.nR, Lt = a.Lt, NB = a.B, D1 = a.tf + 2, n = H * K, bw = sdepth_bandwidth(H, K, a.tf), R1 = bw + 1;
  const int s = blockIdx.x / a.M, j = blockIdx.x - s * a.M;
  double* B = lds;                      // [n][R1] the band of Q, then of L
  double* xv = B + (size_t)n * R1;      // [n] v, the state
  double* rm = xv + n;                  // [n] rhs -> L^-1 rhs -> m
  double* ru = rm + n;                  // [n] z -> nu = L^-T z
  double* xp = ru + n;                  // [n] v', the proposal
  double* bv = xp + n;                  // [n] b
  double* invd = bv + n;                // [n] 1 / L_ii
  double* A = invd + n;                 // [H][KK] packed lower triangles of A_h
  double* tau = A + (size_t)H * KK;     // [nR] x 4: tau2, c, b, a
  double* lc = tau + nR;
  double* lb = lc + nR;
  double* la = lb + nR;
  double* itau = la + nR;               // [nR] 1 / (lam2 tau2)
  double* off = itau + nR;              // [nR][K] D_o V_s[j]
  double* pb = off + (size_t)nR * K;    // [H][D1] the prior band: entry (h + d, h)
  double* vt = pb + (size_t)H * D1;     // [Lt][K] the kept tail
  unsigned short* ptab = reinterpret_cast<unsigned short*>(vt + (size_t)Lt * K);
  const unsigned long long sg = (unsigned long long)(a.sample0 + s);
  const unsigned long long stream = (sg << 32) | (unsigned long long)(unsigned)j;
  const size_t chain = (size_t)s * a.M + j;
  const int per = n + 1 + a.max_rounds + 4 * nR;                      // one sweep's record
  const size_t LD = (size_t)4 * nR + (size_t)a.sweeps * per;
  const double* dr = a.draws ? a.draws + chain * LD : nullptr;
  const double lam2 = a.lam2[(size_t)s * a.lstride];
  const double lo = a.lo, hi = a.hi;
  const bool fixed = a.tau2 != nullptr;
  const LikFam lf{a.fam, a.par};
  auto clip = [&](double x) { return fmin(fmax(x, lo), hi); };
  const double* __restrict__ W = a.W + (size_t)s * N * K;
  const size_t col = (size_t)j * H * N;                                // this column's statistics
  const int* __restrict__ rows = a.ridx + a.rptr[j];
  const int nr = a.rptr[j + 1] - a.rptr[j];

  fill_pair_table(ptab, bw);
  // ---- the kept tail and the offsets D_o V_s[j]: row r reaches depths rcol0 + e < 0, tail index Lt + rcol0 + e
  {
    const double* __restrict__ src = a.Vtail + chain * (size_t)a.vstride;
    for (int idx = lane; idx < Lt * K; idx += WAVE) vt[idx] = src[idx];
    __syncthreads();
    for (int idx = lane; idx < nR * K; idx += WAVE) {
      const int r = idx / K, k = idx - r * K, t0 = a.rcol0[r];
      double sum = 0.0;
      for (int e = 0; e < D1; ++e) {
        const int t = t0 + e;
        if (t < 0 && Lt + t >= 0) sum = fma(a.rcoef[(size_t)r * D1 + e], vt[(Lt + t) * K + k], sum);
      }
      off[idx] = sum;
    }
  }
  // ---- A_h and b_h of the fit, lanes along rows, every new depth in turn (the accumulation of slice_fold_cols_kernel)
  for (int h = 0; h < H; ++h) {
    const double* __restrict__ fa = a.fa + col + (size_t)h * N;
    const double* __restrict__ fb = a.fb + col + (size_t)h * N;
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
      for (int e = 0; e < KK; ++e) A[(size_t)h * KK + e] = acc[e];
#pragma unroll
      for (int k = 0; k < K; ++k) bv[h * K + k] = acc[KK + k];
    }
  }
  // ---- the start: the levels (sample_horseshoe_plus, Tau2 clipped as _init_Tau2 does; or the fixed scales) and v
  for (int r = lane; r < nR; r += WAVE) {
    if (fixed) { tau[r] = a.tau2[chain * nR + r]; la[r] = lb[r] = lc[r] = 1.0; continue; }
    double g0[4];
    if (dr) {
#pragma unroll
      for (int q = 0; q < 4; ++q) g0[q] = dr[(size_t)q * nR + r];
    } else {
      CellRng g = sdepth_rng(a.seed, stream, 0, r);
#pragma unroll
      for (int q = 0; q < 4; ++q) g0[q] = gamma_mt(0.5, g);
    }
    const double av = 1.0 / g0[0], bq = 1.0 / (av * g0[1]), cv = 1.0 / (bq * g0[2]);
    la[r] = av; lb[r] = bq; lc[r] = cv;
    tau[r] = fmin(1.0 / (cv * g0[3]), SDEPTH_TAU2_START_CLIP);
  }
  {
    const double* __restrict__ st = a.start ? a.start + chain * (size_t)n : nullptr;
    double* __restrict__ V0 = a.Vstart + chain * (size_t)n;
    for (int idx = lane; idx < n; idx += WAVE) {
      const double x = st ? st[idx] : vt[(Lt - 1) * K + idx % K];        // (the last kept depth, bit for bit)
      xv[idx] = x;
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
      const double* kept = vt + (size_t)(Lt - NB) * K;
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
  // number `pos` of the uniforms of sweep `sw` (0: u_h, 1: u_a, 2 + rd: the shrink uniforms)
  auto uniform = [&](int sw, int pos) {
    if (dr) return dr[(size_t)4 * nR + (size_t)sw * per + n + pos];
    CellRng g = sdepth_rng(a.seed, stream, sw + 1, nR + n + pos);
    return g.uniform();
  };

  const double bad = __builtin_nan("");
  double* __restrict__ Vo = a.V + chain * n;
  double* __restrict__ To = a.Tau2 + chain * nR;
  const int fail_id = (int)(sg * (unsigned long long)a.M + (unsigned)j);
  double ll = feasible(xv) ? ratio(xv) : bad;
  if (!(fabs(ll) < INFINITY)) {                // (false for nan too)
    for (int idx = lane; idx < n; idx += WAVE) Vo[idx] = bad;
    for (int r = lane; r < nR; r += WAVE) To[r] = bad;
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
    const double* ds = dr ? dr + (size_t)4 * nR + (size_t)sw * per : nullptr;
    if (sw == 0 || !fixed) {
      // ---- the prior band from 1 / (lam2 tau2), then the band of Q: column nn = h K + k holds the entries (nn + o, nn)
      for (int r = lane; r < nR; r += WAVE) itau[r] = 1.0 / (lam2 * tau[r]);
      __syncthreads();
      for (int e0 = lane; e0 < H * D1; e0 += WAVE) {
        double sum = 0.0;
        for (int e = a.st_ptr[e0]; e < a.st_ptr[e0 + 1]; ++e) sum = fma(a.st_coef[e], itau[a.st_row[e]], sum);
        pb[e0] = sum;
      }
      __syncthreads();
      for (int idx = lane; idx < n * R1; idx += WAVE) {
        const int nn = idx / R1, o = idx - nn * R1;
        const int h = nn / K, k = nn - h * K;
        const int row = nn + o, h2 = row / K, k2 = row - h2 * K;
        double v = 0.0;
        if (row < n) {
          if (h2 == h) v = A[(size_t)h * KK + lidx(k2, k)];
          if (k2 == k) v += pb[h * D1 + (h2 - h)];
        }
        B[idx] = v;
      }
      // ---- rhs = b - D_n' diag(1 / (lam2 tau2)) off (rows of R in ascending order)
      for (int idx = lane; idx < n; idx += WAVE) {
        const int h = idx / K, k = idx - h * K;
        double sum = 0.0;
        for (int r = 0; r < nR; ++r) {
          const int e = h - a.rcol0[r];
          if (e >= 0 && e < D1) sum = fma(a.rcoef[(size_t)r * D1 + e] * itau[r], off[r * K + k], sum);
        }
        rm[idx] = bv[idx] - sum;
      }
      __syncthreads();
      // ---- Q = L L', rm = L^-1 rhs, then m = L^-T rm
      ok = banded_factor_forward(B, rm, invd, ptab, n, bw);
      if (!ok) break;
      __syncthreads();
      banded_backward(B, rm, invd, n, bw);
    }
    for (int idx = lane; idx < n; idx += WAVE) {
      double z;
      if (ds) z = ds[idx];
      else { CellRng g = sdepth_rng(a.seed, stream, sw + 1, nR + idx); z = g.normal(); }
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
    // ---- the levels, lane = new penalty row: dv = off + D_n v
    for (int r = lane; r < nR; r += WAVE) {
      const int t0 = a.rcol0[r];
      double dv[K];
#pragma unroll
      for (int k = 0; k < K; ++k) dv[k] = off[r * K + k];
      for (int e = 0; e < D1; ++e) {
        const int t = t0 + e;
        if (t < 0 || t >= H) continue;                       // a kept depth (in off), or past the grid (coefficient 0)
        const double cf = a.rcoef[(size_t)r * D1 + e];
#pragma unroll
        for (int k = 0; k < K; ++k) dv[k] = fma(cf, xv[t * K + k], dv[k]);
      }
      double dsq = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) dsq = fma(dv[k], dv[k], dsq);
      double g4[4];
      if (ds) {
#pragma unroll
        for (int q = 0; q < 4; ++q) g4[q] = ds[(size_t)n + 1 + a.max_rounds + (size_t)q * nR + r];
      } else {
        CellRng g = sdepth_rng(a.seed, stream, sw + 1, r);
        g4[0] = gamma_mt(0.5 * (K + 1), g);
#pragma unroll
        for (int q = 1; q < 4; ++q) g4[q] = gamma_mt(1.0, g);
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
  for (int r = lane; r < nR; r += WAVE) To[r] = ok ? tau[r] : bad;
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
#endif  // BTF_SLICE_FOLD_DEPTH_UNIT
