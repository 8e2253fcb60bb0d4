// Folding new rows into a slice-sampled fit  (counted under BTF_K_CRITERIA)
//
// The row prior of both slice-sampled models is N(0, sigma2 I) (factor.py:685-686); a NEW row lies beyond the leading K
// rows, so the lower-triangular restriction does not touch it.  Given V_s (and U_s) every restriction on the row is linear
// in w - the curve constraints  sum_t A[c,t] (w . v_jt) >= C[c]  of every column, the fixed row constraints, and
// 0 <= w . u_f <= 1 - so the feasible set is convex, and elliptical slice sampling (elliptical_slice.py:59-124, mu = 0)
// with the constraints as a likelihood of minus infinity is a valid sampler of p(w_new | y_new, V_s, U_s): every proposal
// lies on an ellipse through the current feasible state, and the bracket shrinks towards it.
// functionalmf_amd/slice_fold_in.py restates the chain in numpy; that module is the definition.
//
// ONE launch, slice_fold_kernel<K, LINK>, covers all samples, all rows and all sweeps; nothing is read back in between.
//   layout       one wave owns one chain (sample s, row r) from its start to its last sweep; a workgroup holds SF_CHAINS
//                consecutive chains, which share the LDS tables (log or exp table of btf_device.h; gamma grid: gg_stage's
//                table).  The tables are staged behind the ONE barrier of the kernel; after it the waves never meet again
//                (they finish at different times).
//   state        x, nu, x' are wave-uniform: every lane holds the same values, so acceptance and shrinking are too.
//   likelihood   lanes run along the cells (j,t): lane l takes cells l, l + 64, ... in ascending order (row statistics
//                [R][MT]: coalesced), the 64 lane sums are combined by the xor butterfly of wave_sum - every lane ends
//                with the same bits.  The feature term runs over lanes the same way (lanes over f).
//   feasibility  lanes over (column, constraint) pairs, Constraints_A walked by its non-zeros (CSR), then lanes over the
//                row constraints and over the features; a wave vote.  Tested first: an infeasible proposal costs no
//                likelihood pass.
//   draws        one sweep consumes a record of K + 1 + max_rounds numbers: K normals, u_h, u_a, the shrink uniforms.
//                Given (`draws`), or Philox keyed (seed, stream = global sample index << 32 | row,
//                index = sweep * record length + position) - never a thread or block index.  A result does not depend on
//                the grid, on how many rows or samples a call holds, or on where the states come from.  No float atomics.
//   bounded      sweeps * max_rounds proposals per chain; no spin-waits, no communication between workgroups.
//   bad start    infeasible, or a non-finite likelihood: NaN for that chain, the status flag, and the smallest failing
//                sample * R + row by integer atomicMin; the chain does not run.
// slice_fold_mean_kernel: the default start w0_s = mean of the N rows of W_s, summed in row order.
#pragma once
#include "btf_device.h"
#include "btf_gamma_grid.h"

namespace btf {

constexpr int SF_CHAINS = 4;                   // chains (waves) per workgroup (geometry only)

struct SliceFoldArgs {
  const double* V;                             // [S][MT][K]
  const double* start; long long st_s, st_r;   // start of chain (s, r) at start[s * st_s + r * st_r + k]
  const double* sigma2; int sstride;           // sigma2 of sample s at sigma2[s * sstride]
  const double* S1; const double* cnt; const double* L;    // [R][MT]; L: gamma grid only
  const int* cs_ptr; const int* cs_idx; const double* cs_val; const double* Cc; int J;    // curve constraints, CSR over [J][T]
  const double* Rc; int nrc;                   // [nrc][K+1]
  const double* U; int F;                      // [S][F][K]
  const unsigned char* codes;                  // [R][F]: 0, 1, 2 = missing
  const double* draws;                         // [S][R][sweeps][K + 1 + max_rounds], or null: the device generator
  const GgComp* gg; int G; double lsp;         // gamma grid: the component table
  int fam; double par;                         // ESS_LINK_GENERIC: the family and its parameter
  double* W;                                   // [S][R][K]
  int* rounds; int* unfinished;                // [S][R]
  int* status;                                 // [0]: 1 after a bad start, [1]: the smallest failing sample * R + row
  unsigned long long seed;
  long long sample0;                           // global index of sample 0 of this call (generator keys)
  int S, R, M, T, sweeps, max_rounds;
};

// the kernels live in btf_slice_fold.hip (a compilation unit of their own); the C-ABI unit launches them through these
using SliceFoldKernel = void (*)(SliceFoldArgs);
using SliceFoldMeanKernel = void (*)(const double*, int, int, int, double*);
SliceFoldKernel slice_fold_fn(int K, int family);     // null outside K = 1..10, family = 0..5 (ESS_FAM_*)
SliceFoldMeanKernel slice_fold_mean_fn();

}  // namespace btf

#ifdef BTF_SLICE_FOLD_UNIT
namespace btf {

// out[s][k] = (sum_i W[s][i][k]) / N, the rows added in ascending order
static __global__ void slice_fold_mean_kernel(const double* __restrict__ W, int S, int N, int K, double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)S * K) return;
  const long long s = e / K;
  const int k = (int)(e - s * K);
  double sum = 0.0;
  for (int i = 0; i < N; ++i) sum += W[((size_t)s * N + i) * K + k];
  out[e] = sum / (double)N;
}

template <int K, int LINK>
__global__ __launch_bounds__(SF_CHAINS * WAVE) void slice_fold_kernel(SliceFoldArgs a) {
  constexpr bool GG = LINK == ESS_LINK_GAMMA_GRID;
  __shared__ double2 ltab[LINK == ESS_LINK_GENERIC ? 1 : LOGTAB_N];
  __shared__ double2 etab[GG ? LOGTAB_N : 1];
  __shared__ GgComp tab[GG ? GG_MAXG : 1];
  if constexpr (GG) gg_stage(GgTab{nullptr, a.gg, a.G, a.lsp}, tab, ltab, etab);
  else if constexpr (LINK == ESS_LINK_IDENTITY) log_table_build(ltab);
  else if constexpr (LINK == ESS_LINK_LOG) exp_table_build(ltab);
  __syncthreads();                              // the only barrier: from here on every wave is on its own
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const long long chain = (long long)blockIdx.x * SF_CHAINS + wv;
  if (chain >= (long long)a.S * a.R) return;
  const int R = a.R, MT = a.M * a.T, F = a.F;
  const int s = (int)(chain / R), r = (int)(chain - (long long)s * R);
  const double* __restrict__ V = a.V + (size_t)s * MT * K;
  const double* __restrict__ S1 = a.S1 + (size_t)r * MT;
  const double* __restrict__ cnt = a.cnt + (size_t)r * MT;
  const double* __restrict__ Lr = GG ? a.L + (size_t)r * MT : nullptr;
  const double* __restrict__ U = F ? a.U + (size_t)s * F * K : nullptr;
  const unsigned char* __restrict__ codes = F ? a.codes + (size_t)r * F : nullptr;
  const unsigned long long sg = (unsigned long long)(a.sample0 + s);
  const unsigned long long stream = (sg << 32) | (unsigned long long)(unsigned)r;
  const int rec = K + 1 + a.max_rounds;
  const LikFam lf{a.fam, a.par};

  auto dot = [&](const double (&w)[K], const double* __restrict__ v) {
    double e = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) e = fma(w[k], v[k], e);
    return e;
  };
  // every restriction holds at w (a wave vote; NaN fails every comparison)
  auto feasible = [&](const double (&w)[K]) -> bool {
    bool ok = true;
    const int ncon = a.M * a.J;
    for (int q = lane; q < ncon; q += WAVE) {
      const int j = q / a.J, c = q - j * a.J;
      double acc = 0.0;
      for (int e = a.cs_ptr[c]; e < a.cs_ptr[c + 1]; ++e)
        acc = fma(a.cs_val[e], dot(w, V + ((size_t)j * a.T + a.cs_idx[e]) * K), acc);
      ok = ok && acc >= a.Cc[c];
    }
    for (int q = lane; q < a.nrc; q += WAVE) {
      const double* __restrict__ row = a.Rc + (size_t)q * (K + 1);
      ok = ok && dot(w, row) >= row[K];
    }
    for (int f = lane; f < F; f += WAVE) {
      const double p = dot(w, U + (size_t)f * K);
      ok = ok && p >= 0.0 && p <= 1.0;
    }
    return __all(ok ? 1 : 0) != 0;
  };
  // log-likelihood of the row at w plus the feature term; the same bits in every lane
  auto loglik = [&](const double (&w)[K]) -> double {
    double sum = 0.0;
    for (int cell = lane; cell < MT; cell += WAVE) {
      const double eta = dot(w, V + (size_t)cell * K);
      if constexpr (GG) sum += gg_term(S1[cell], Lr[cell], cnt[cell], eta, tab, a.G, a.lsp, ltab, etab);
      else sum += poisson_term<LINK>(S1[cell], cnt[cell], eta, ltab, lf);
    }
    sum = wave_sum(sum);
    if (F) {
      double t = 0.0;
      for (int f = lane; f < F; f += WAVE) {
        const int code = codes[f];
        const double p = dot(w, U + (size_t)f * K);
        t += code == 2 ? 0.0 : log(code == 1 ? p : 1.0 - p);
      }
      sum += wave_sum(t);
    }
    return sum;
  };
  // number `pos` of the chain's record of sweep `sw`: given, or Philox (normals and uniforms on counters of their own)
  const double* __restrict__ given = a.draws ? a.draws + (size_t)chain * a.sweeps * rec : nullptr;
  auto normal = [&](int sw, int pos) {
    const unsigned long long idx = (unsigned long long)sw * rec + pos;
    return given ? given[idx] : philox_normal(a.seed, stream, idx);
  };
  auto uniform = [&](int sw, int pos) {
    const unsigned long long idx = (unsigned long long)sw * rec + pos;
    if (given) return given[idx];
    uint32_t w4[4];
    Philox::gen(a.seed, stream, (1ULL << 62) + idx, w4);
    return u01(w4[0], w4[1]);
  };

  double x[K], nu[K], xp[K];
  const double* __restrict__ st = a.start + (size_t)s * a.st_s + (size_t)r * a.st_r;
#pragma unroll
  for (int k = 0; k < K; ++k) x[k] = st[k];
  double* __restrict__ wo = a.W + (size_t)chain * K;
  double ll = feasible(x) ? loglik(x) : __builtin_nan("");
  if (!(fabs(ll) < INFINITY)) {                // (false for nan too)
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) wo[k] = __builtin_nan("");
      a.rounds[chain] = 0; a.unfinished[chain] = 0;
      a.status[0] = 1;
      atomicMin(&a.status[1], (int)(sg * (unsigned long long)R + (unsigned)r));
    }
    return;
  }
  const double sd = sqrt(a.sigma2[(size_t)s * a.sstride]);
  const double two_pi = 6.283185307179586476925286766559;
  int nrounds = 0, nunf = 0;
  for (int sw = 0; sw < a.sweeps; ++sw) {
#pragma unroll
    for (int k = 0; k < K; ++k) nu[k] = sd * normal(sw, k);
    const double hh = ll + log(uniform(sw, K));
    double phi = two_pi * uniform(sw, K + 1);
    double lo = phi - two_pi, hi = phi;
    bool accepted = false;
    for (int rd = 0; rd < a.max_rounds; ++rd) {
      double sn, cs;
      sincos(phi, &sn, &cs);
#pragma unroll
      for (int k = 0; k < K; ++k) xp[k] = fma(x[k], cs, nu[k] * sn);
      if (feasible(xp)) {
        ++nrounds;
        const double llp = loglik(xp);
        if (llp >= hh) {
#pragma unroll
          for (int k = 0; k < K; ++k) x[k] = xp[k];
          ll = llp;
          accepted = true;
          break;
        }
      }
      if (phi > 0.0) hi = phi; else lo = phi;
      if (rd + 1 < a.max_rounds) phi = fma(hi - lo, uniform(sw, K + 2 + rd), lo);
    }
    if (!accepted) ++nunf;                     // the cap: the sweep keeps x
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) wo[k] = x[k];
    a.rounds[chain] = nrounds;
    a.unfinished[chain] = nunf;
  }
}

}  // namespace btf
#endif  // BTF_SLICE_FOLD_UNIT
