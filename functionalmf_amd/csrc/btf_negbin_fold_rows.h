// Folding new rows into a fitted Negative-Binomial posterior, with a fixed or a SAMPLED rate  (counted under BTF_K_CRITERIA)
//
// Reference: given the rate the Negative-Binomial model is the Binomial one on pseudo-data (factor.py:506-511, 553): a cell
// with c observed replicates, their sum ysum and rate r draws omega ~ PG(ysum + c r, w . v_jt) and has kappa = (ysum - c r) / 2.
// A new row runs the chain of fold_in_kernel's Binomial family on them, from w = 0 with the prior N(0, sigma2 I).  Where
// the fit has one rate per row (rdims = (1, 2)) a new row has no kept rate; the chain then samples one scalar rate for it
// with the model's own random-walk Metropolis step on log r (_resample_R, factor.py:513-554, restricted to the one row) in
// front of every sweep - the order of the model's resample: rate, weights, w.  functionalmf_amd/negbin_fold_in.py
// (chain_rows) is the definition in numpy.
//
// ONE launch, negbin_fold_rows_kernel<K, SAMPLED>, with the geometry of fold_in_kernel: a workgroup of FOLD_PARTS waves owns
// (sample s, 64 new rows) for all sweeps, lane = row; wave p takes the cells jt = p, p + FOLD_PARTS, ... in ascending
// order; the parts of a row are added in part order through LDS, ((p0 + p1) + p2) + p3; no floating-point atomics; a
// result never depends on the grid, on how many rows or samples a call holds.  Per sweep:
//   pass A (SAMPLED)  psi = w . v_jt per cell and the running L = sum c log(1 - P), P = ilogit(clip(psi, -10, 10)), as
//       -c log1p(exp(clip psi)); the parts added in part order.
//   Metropolis        wave 0, one row per lane, nmetropolis steps with L held (w does not move): cand = exp(log r +
//       rpropstdev n), prior = (log^2 r - log^2 cand) / (2 rstdev^2), ll = sum over the row's histogram of
//       h [rise(y, cand) - rise(y, r)] + (cand - r) L with rise = nb_lgamma_rise (btf_lgamma.h), accept when
//       u <= exp(clip(prior + ll, -10, 1)) and cand > 1 - the arithmetic of nb_mh_step_kernel (btf_kernels.h), the state kept
//       as (log r, r).  The histogram lies [bin][row] (one coalesced load per bin), padded with h = 0.  The rate goes back
//       to all waves through LDS.
//   pass B            psi again, omega by the sampler of the model's sweeps (pg_draw_series below PG_NORMAL_B, pg_draw_normal
//       from there on) on a CellRng keyed (a Philox word of (seed, sample, row), sweep * MT + jt), then the K (K + 1) / 2 + K
//       running sums.  The weights of NBROWS_OM_CELLS cells per lane are drawn into LDS first and accumulated from there,
//       so that the series sampler's generator and candidate loop are not live inside the multiply-add loop (negbin_draw_depth
//       of btf_fold_chain.h does the same per depth).  The fixed rate is read through strides (sample, row, column, depth;
//       0 = shared).  A missing cell (c = 0) draws nothing and adds exact zeros.
//   solve and draw    wave 0: the packed Cholesky and the draw of fold_in_kernel.
// Generators: Philox keyed (seed, stream = global sample index << 32 | row) - never a thread or block index.  Counters of a
// stream: the K normals of sweep sw at normal index sw K + k (counter (sw K + k) / 2, below 2^40); the Polya-Gamma key at
// counter 0x666f6c64 << 24 (about 2^54.7; the cells then count on a key of their own); the Metropolis pair q = sw nmetropolis
// + step at counters 2^59 + 2 q (normal) and 2^59 + 2 q + 1 (uniform).  sweeps and nmetropolis stay below 2^20.
// Replay inputs z, mh and omega replace every generator.
// Failures: a non-positive pivot - which a psi that is not finite or lies beyond 1e8 forces through a nan weight - raises
// status[0] and leaves the smallest failing (global sample) * R + row in status[1] (integer atomicMin); the row is nan.
// fp64 throughout (the series sampler's candidates are f32, as in the sampler's sweeps).
#pragma once
#include "btf_fold_in.h"

namespace btf {

constexpr int NBROWS_OM_CELLS = 8;                          // cells per lane whose weights wait in LDS for the accumulation
constexpr unsigned long long NBROWS_MH_INDEX = 1ULL << 60;  // normal index of the first Metropolis pair (Philox counter 2^59)
constexpr unsigned long long NBROWS_PG_COUNTER = 0x666f6c64ULL << 24;   // the Polya-Gamma key's counter (fold_in_kernel's)
constexpr int NBROWS_MAX_STEPS = 1 << 20;                   // sweeps and nmetropolis: keeps the counter ranges apart

struct NegbinFoldRowsArgs {
  const double* V;          // [S][MT][K]
  const double* sigma2;     // [S]
  const double* cnt;        // [MT][R] observed replicates of the cell
  const double* ysum;       // [MT][R] their sum
  const double* rate;       // fixed rate of (s, row, column j, depth t) at rate[s rs_s + row rs_r + j rs_j + t rs_t]
  long long rs_s, rs_r, rs_j, rs_t;
  const double* rate0;      // [S][R] the start of a sampled rate
  const double* hy;         // [B][R] the distinct counts of a row ...
  const double* hn;         // [B][R] ... and how often each was observed (0: padding)
  const double* omega;      // [S][sweeps][MT][R] weights in the place of every Polya-Gamma draw, or null
  const double* z;          // [S][R][sweeps][K] standard normals, or null: the device generator
  const double* mh;         // [S][R][sweeps][2][nm] normals, then uniforms of the Metropolis steps, or null
  double* W;                // [S][R][K]
  double* Wmean;            // [S][R][K]
  double* Rout;             // [S][R] the rate at the last sweep (sampled)
  double* accept;           // [S][R] accepted share of the chain's Metropolis steps (sampled)
  int* status;              // [0]: 1 after a failure, [1]: the smallest failing sample * R + row
  unsigned long long seed;
  long long sample0;        // global index of sample 0 of this call (generator keys)
  double rprop, rstdev;
  int S, R, T, MT, B, nm, sweeps;
};

using NegbinFoldRowsKernel = void (*)(NegbinFoldRowsArgs);
NegbinFoldRowsKernel negbin_fold_rows_fn(int K, int sampled);      // null outside K = 1..10 (btf_fold_in.hip)

}  // namespace btf

#ifdef BTF_FOLD_UNIT
#include "btf_kernels.h"        // CellRng, pg_draw_series / pg_draw_normal, PG_NORMAL_B; btf_lgamma.h

namespace btf {

template <int K, bool SAMPLED>
__global__ __launch_bounds__(FOLD_PARTS * WAVE) void negbin_fold_rows_kernel(NegbinFoldRowsArgs a) {
  constexpr int KK = tri(K), NA = KK + K, NT = FOLD_PARTS * WAVE, CB = NBROWS_OM_CELLS;
  __shared__ double red[NA][WAVE];
  __shared__ double wsh[K][WAVE];
  __shared__ double rsh[WAVE];
  __shared__ double om[CB][NT];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int s = blockIdx.x, R = a.R, MT = a.MT, T = a.T;
  const int r = blockIdx.y * WAVE + lane;
  const bool row_ok = r < R;
  const int rc = row_ok ? r : R - 1;                         // clamped row for the loads of the lanes past the end
  const double* __restrict__ V = a.V + (size_t)s * MT * K;
  const double* __restrict__ cnt = a.cnt + rc;
  const double* __restrict__ ysum = a.ysum + rc;
  const double* __restrict__ rate = SAMPLED ? nullptr : a.rate + (long long)s * a.rs_s + (long long)rc * a.rs_r;
  const unsigned long long sg = (unsigned long long)(a.sample0 + s);
  const unsigned long long stream = (sg << 32) | (unsigned long long)(unsigned)r;
  unsigned long long pg_key = 0;
  if (!a.omega) {
    uint32_t kw[4];
    Philox::gen(a.seed, stream, NBROWS_PG_COUNTER, kw);
    pg_key = ((unsigned long long)kw[1] << 32) | kw[0];
  }
  double w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = 0.0;
  double rr = 1.0, logr = 0.0;                               // the sampled rate of this lane's row
  if constexpr (SAMPLED) { rr = a.rate0[(size_t)s * R + rc]; logr = log(rr); }
  int nacc = 0;
  bool failed = false;
  for (int sw = 0; sw < a.sweeps; ++sw) {
    if constexpr (SAMPLED) {
      // ---- pass A: L = sum c log(1 - P) over this wave's cells, ascending
      double Lp = 0.0;
      for (int jt = wv; jt < MT; jt += FOLD_PARTS) {
        double psi = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) psi = fma(w[k], V[(size_t)jt * K + k], psi);
        const double c = cnt[(size_t)jt * R];
        if (c > 0.0) Lp -= c * log1p(exp(fmin(fmax(psi, -10.0), 10.0)));
      }
      for (int p = 1; p < FOLD_PARTS; ++p) {
        __syncthreads();
        if (wv == p) red[0][lane] = Lp;
        __syncthreads();
        if (wv == 0) Lp += red[0][lane];
      }
      // ---- the Metropolis steps on log r (factor.py:522-550): wave 0, one row per lane
      if (wv == 0) {
        const double* __restrict__ mhp = a.mh ? a.mh + (((size_t)s * R + rc) * a.sweeps + sw) * 2 * (size_t)a.nm : nullptr;
        const double inv2s = 1.0 / (2.0 * a.rstdev * a.rstdev);
        for (int step = 0; step < a.nm; ++step) {
          const unsigned long long q = (unsigned long long)sw * a.nm + step;
          double n, u;
          if (mhp) { n = mhp[step]; u = mhp[a.nm + step]; }
          else {
            n = philox_normal(a.seed, stream, NBROWS_MH_INDEX + 4ULL * q);
            uint32_t uw[4];
            Philox::gen(a.seed, stream, (NBROWS_MH_INDEX >> 1) + 2ULL * q + 1ULL, uw);
            u = u01(uw[0], uw[1]);
          }
          const double cl = logr + a.rprop * n;
          const double c = exp(cl);
          const double prior = (logr * logr - cl * cl) * inv2s;
          double ll = 0.0;
          for (int b = 0; b < a.B; ++b) {
            const double h = a.hn[(size_t)b * R + rc], y = a.hy[(size_t)b * R + rc];
            if (h > 0.0 && y > 0.0) ll += h * (nb_lgamma_rise(y, c) - nb_lgamma_rise(y, rr));
          }
          ll += (c - rr) * Lp;
          const double prob = exp(fmin(fmax(prior + ll, -10.0), 1.0));
          if (u <= prob && c > 1.0) { logr = cl; rr = c; ++nacc; }      // the floor is the model's own (factor.py:547)
        }
        rsh[lane] = rr;
      }
      __syncthreads();
      rr = rsh[lane];
    }
    // ---- pass B: the weights of a block of cells into LDS, then their sums; this wave's cells, ascending
    double acc[NA];
#pragma unroll
    for (int e = 0; e < NA; ++e) acc[e] = 0.0;
    const double* __restrict__ omg = a.omega ? a.omega + ((size_t)s * a.sweeps + sw) * MT * R + rc : nullptr;
    for (int j0 = wv; j0 < MT; j0 += FOLD_PARTS * CB) {
      for (int i = 0; i < CB; ++i) {
        const int jt = j0 + i * FOLD_PARTS;
        if (jt >= MT) break;
        const double c = row_ok ? cnt[(size_t)jt * R] : 0.0;
        double o = 0.0;
        if (c > 0.0) {
          double psi = 0.0;
#pragma unroll
          for (int k = 0; k < K; ++k) psi = fma(w[k], V[(size_t)jt * K + k], psi);
          if (!(fabs(psi) <= 1e8)) o = __builtin_nan("");
          else if (omg) o = omg[(size_t)jt * R];
          else {
            const double rt = SAMPLED ? rr : rate[(long long)(jt / T) * a.rs_j + (long long)(jt % T) * a.rs_t];
            const double b = fma(c, rt, ysum[(size_t)jt * R]);
            CellRng g(pg_key, (unsigned long long)sw * MT + jt);
            o = b >= (double)PG_NORMAL_B ? pg_draw_normal(b, psi, g) : pg_draw_series(b, psi, g);
          }
        }
        om[i][tid] = o;                                      // (read back by this thread alone: no barrier)
      }
#pragma unroll 2
      for (int i = 0; i < CB; ++i) {
        const int jt = j0 + i * FOLD_PARTS;
        if (jt >= MT) break;
        double v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = V[(size_t)jt * K + k];
        const double c = row_ok ? cnt[(size_t)jt * R] : 0.0;
        const double rt = SAMPLED ? rr : rate[(long long)(jt / T) * a.rs_j + (long long)(jt % T) * a.rs_t];
        const double y = c > 0.0 ? 0.5 * (ysum[(size_t)jt * R] - c * rt) : 0.0;      // kappa
        const double wt = om[i][tid];
#pragma unroll
        for (int p = 0; p < K; ++p) {
          const double t = wt * v[p];
          acc[KK + p] = fma(y, v[p], acc[KK + p]);
#pragma unroll
          for (int q = 0; q <= p; ++q) acc[lidx(p, q)] = fma(t, v[q], acc[lidx(p, q)]);
        }
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
      const double inv_s2 = 1.0 / a.sigma2[s];
      double L[KK], m[K], u[K];
#pragma unroll
      for (int e = 0; e < KK; ++e) L[e] = acc[e];
#pragma unroll
      for (int k = 0; k < K; ++k) { L[lidx(k, k)] += inv_s2; m[k] = acc[KK + k]; }
      bool ok = !failed && inv_s2 > 0.0;                     // (false for a sigma2 that is nan or infinite: reported like a pivot)
#pragma unroll
      for (int j = 0; j < K; ++j) {
        double d = L[lidx(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d = fma(-L[lidx(j, k)], L[lidx(j, k)], d);
        ok = ok && d > 0.0;                                  // (false for nan: a non-finite sigma2 / V / psi ends here too)
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
        u[k] = a.z ? a.z[(((size_t)s * R + rc) * a.sweeps + sw) * K + k] : philox_normal(a.seed, stream, (unsigned long long)sw * K + k);
#pragma unroll
      for (int i = K - 1; i >= 0; --i) {
        double x = u[i];
#pragma unroll
        for (int k = i + 1; k < K; ++k) x = fma(-L[lidx(k, i)], u[k], x);
        u[i] = x / L[lidx(i, i)];
      }
#pragma unroll
      for (int k = 0; k < K; ++k) w[k] = ok ? m[k] + u[k] : __builtin_nan("");
      if (!ok && !failed && row_ok) {
        a.status[0] = 1;
        atomicMin(&a.status[1], (int)(sg * (unsigned long long)R + (unsigned)r));
      }
      failed = !ok;
      if (sw + 1 == a.sweeps && row_ok) {
        double* __restrict__ wo = a.W + ((size_t)s * R + r) * K;
        double* __restrict__ mo = a.Wmean + ((size_t)s * R + r) * K;
#pragma unroll
        for (int k = 0; k < K; ++k) { wo[k] = w[k]; mo[k] = ok ? m[k] : __builtin_nan(""); }
        if constexpr (SAMPLED) {
          a.Rout[(size_t)s * R + r] = ok ? rr : __builtin_nan("");
          a.accept[(size_t)s * R + r] = (double)nacc / ((double)a.sweeps * (double)a.nm);
        }
      }
#pragma unroll
      for (int k = 0; k < K; ++k) wsh[k][lane] = w[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = wsh[k][lane];
  }
}

}  // namespace btf
#endif  // BTF_FOLD_UNIT
