// Binary row features in the constrained model (doseresponse/fit.py:40-50 rowcol_likelihood_with_X, :102-145 the U step).
// X [N][F] in {0, 1, missing}, U [F][K]; with p_if = w_i . u_f the rows of W carry the Bernoulli side term
//   sum_f  x_if log p_if + (1 - x_if) log(1 - p_if)                       (np.nansum: a pair outside [0, 1] adds nothing)
// under the derived constraints 0 <= w_i . u_f <= 1, and every u_f is itself a GASS chain: prior N(0, I_K), the 2N
// constraints 0 <= w_i . u_f <= 1, the same term summed over the rows.  The F chains are independent given W.
//
//   gass_feat_rc_kernel        the 2F derived rows (u_f, 0), (-u_f, -1) behind the user's rows of the row-constraint
//                              buffer: gass_analyse_rows_kernel only sees a larger nrc
//   gass_feat_analyse_kernel   one workgroup per feature: x0 = u_f, v = z (given, or Philox), a, b of the two constraint
//                              rows of every row of W straight from global memory, then gass_finish_grid / gass_pick
//   gass_bern_eval_kernel      the side term of every candidate of every chain, lanes = candidates, the four waves split
//                              the chain's cells, cells staged in LDS as (e0, e1[, em], code):
//                                ROWS   chain = row i, cells = features: e0 = x0 . u_f, e1 = nu . u_f (EP: em = mu . u_f),
//                                       added to the ll the likelihood evaluation left
//                                !ROWS  chain = feature f, cells = rows: e0 = w_i . u0, e1 = w_i . v: the whole ll
//                              cur != nullptr: the current state alone (the candidate at angle 0), one value per chain
// Every sum has a fixed order: two calls give identical bits.  The logarithm is libm's (double).
#pragma once
#include "btf_gass.h"

namespace btf {

constexpr uint64_t GASS_FEAT_STREAM = 0x30000ULL;      // Philox stream of the U step's normals (W: 0x20000 + 2 s, V: 0x10001 + 2 s)

struct GassFeatArgs {            // analysis of the feature chains
  const double* U; const double* W; const double* z;      // [F][K], [N][K], [F][K] or nullptr (Philox)
  int N, F, K;
  double* X0; double* Nu;                                 // [F][K], written here
  unsigned char* vmask; int* info;                        // [F][GASS_GRID], [F][2]
  int pick; int ngrid; double* thetas; int* ntheta;
  unsigned long long seed, pseed;                         // normals; subsample
};

struct GassBernArgs {
  const double* X0; const double* Nu; const double* Mu;   // the chains' state / proposal (/ EP centre), [nchains][K]
  const double* Fx;                                       // the fixed factor: U [F][K] for rows, W [N][K] for features
  const unsigned char* codes;                             // [nchains][ncell]: 0, 1, 2 = missing
  int nchains, ncell, K;
  const double* thetas; const int* ntheta; double* ll;    // [nchains][GASS_MAXC]
  double* cur;                                            // [nchains]: the current state's term (thetas / ll unused)
};

using GassFeatRcKernel = void (*)(const double*, int, int, double*);
using GassFeatKernel = void (*)(GassFeatArgs);
using GassBernKernel = void (*)(GassBernArgs);
// btf_gass_ep.hip: the kernels, for Prof::launch in btf_abi.hip
GassFeatRcKernel gass_feat_rc_fn();
GassFeatKernel gass_feat_analyse_fn();
GassBernKernel gass_bern_eval_fn(bool rows, bool ep);

#ifdef BTF_GASS_EP_UNIT
// rows [2F][K+1]: (u_f, 0) for f < F, then (-u_f, -1)
__global__ void gass_feat_rc_kernel(const double* __restrict__ U, int F, int K, double* __restrict__ rows) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 2 * F * (K + 1)) return;
  const int r = e / (K + 1), k = e - r * (K + 1);
  const bool neg = r >= F;
  const int f = neg ? r - F : r;
  rows[e] = k < K ? (neg ? -U[(size_t)f * K + k] : U[(size_t)f * K + k]) : (neg ? -1.0 : 0.0);
}

__global__ __launch_bounds__(GASS_THREADS) void gass_feat_analyse_kernel(GassFeatArgs a) {
  __shared__ GassScratch S;
  const int f = blockIdx.x, tid = threadIdx.x, K = a.K;
  for (int g = tid; g < GASS_GRID + 8; g += GASS_THREADS) S.diff[g] = 0;
  double x[EIG_MAXK], v[EIG_MAXK];
#pragma unroll
  for (int k = 0; k < EIG_MAXK; ++k) {
    x[k] = 0.0; v[k] = 0.0;
    if (k < K) {
      const size_t o = (size_t)f * K + k;
      x[k] = a.U[o];
      v[k] = a.z ? a.z[o] : philox_normal(a.seed, GASS_FEAT_STREAM, (unsigned long long)o);
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < EIG_MAXK; ++k) if (k < K) { a.X0[(size_t)f * K + k] = x[k]; a.Nu[(size_t)f * K + k] = v[k]; }
  }
  __syncthreads();
  double tmin = -INFINITY, tmax = INFINITY;
  int any = 0;
  for (int i = tid; i < a.N; i += GASS_THREADS) {
    const double* __restrict__ w = a.W + (size_t)i * K;
    double aa = 0.0, bb = 0.0;
#pragma unroll
    for (int k = 0; k < EIG_MAXK; ++k) if (k < K) { aa = fma(w[k], x[k], aa); bb = fma(w[k], v[k], bb); }
    gass_constraint(aa, bb, 0.0, S.diff, tmin, tmax, any);          //  w_i . u >= 0
    gass_constraint(-aa, -bb, -1.0, S.diff, tmin, tmax, any);       // -w_i . u >= -1
  }
  __syncthreads();
  unsigned char* vm = a.vmask + (size_t)f * GASS_GRID;
  const int total = gass_finish_grid(S, tmin, tmax, any, vm, a.info + 2 * f, a.pick != 0, S.diff);
  if (a.pick) gass_pick(total, (any_of(S) & 1) ? 0 : 1, a.ngrid, S.diff, a.thetas + (size_t)f * GASS_MAXC, a.ntheta + f, a.pseed, (unsigned long long)f);
}

// one pair: nothing when missing or p outside [0, 1] (NaN included); log p for x = 1, log(1 - p) for x = 0 (-inf at the edge)
__device__ __forceinline__ double bern_term(double p, int code) {
  const bool ok = code != 2 && p >= 0.0 && p <= 1.0;
  return log(ok ? (code == 1 ? p : 1.0 - p) : 1.0);
}

template <bool ROWS, bool EP>
__global__ __launch_bounds__(GASS_THREADS) void gass_bern_eval_kernel(GassBernArgs a) {
  __shared__ double e0s[GASS_CT], e1s[GASS_CT];
  __shared__ double ems[EP ? GASS_CT : 1];
  __shared__ int cds[GASS_CT];
  __shared__ double red[GASS_THREADS / WAVE][GASS_MAXC];
  const int ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = a.K;
  const bool current = a.cur != nullptr;
  const int nth = current ? 1 : a.ntheta[ch];
  double c0 = 1.0, s0 = 0.0, c1 = 1.0, s1 = 0.0;
  if (!current) {
    const double th0 = lane < nth ? a.thetas[(size_t)ch * GASS_MAXC + lane] : 0.0;
    const double th1 = lane + 64 < nth ? a.thetas[(size_t)ch * GASS_MAXC + lane + 64] : 0.0;
    sincos(th0, &s0, &c0);
    sincos(th1, &s1, &c1);
  }
  const bool two = nth > 64;                     // (uniform over the workgroup)
  __shared__ double xs[EP ? 3 : 2][EIG_MAXK];      // the chain's x0, nu (, mu): read as LDS broadcasts while the cells are staged
  if (tid < K) {
    xs[0][tid] = a.X0[(size_t)ch * K + tid];
    xs[1][tid] = a.Nu[(size_t)ch * K + tid];
    if constexpr (EP) xs[2][tid] = a.Mu[(size_t)ch * K + tid];
  }
  double acc0 = 0.0, acc1 = 0.0;
  const int ncell = a.ncell;
  for (int base = 0; base < ncell; base += GASS_CT) {
    __syncthreads();
    for (int e = tid; e < GASS_CT; e += GASS_THREADS) {
      const int cell = base + e;
      double d0 = 0.0, d1 = 0.0, dm = 0.0;
      int code = 2;
      if (cell < ncell) {
        const double* __restrict__ fx = a.Fx + (size_t)cell * K;
        for (int k = 0; k < K; ++k) {
          d0 = fma(xs[0][k], fx[k], d0); d1 = fma(xs[1][k], fx[k], d1);
          if constexpr (EP) dm = fma(xs[2][k], fx[k], dm);
        }
        code = a.codes[(size_t)ch * ncell + cell];
      }
      e0s[e] = d0; e1s[e] = d1; cds[e] = code;
      if constexpr (EP) ems[e] = dm;
    }
    __syncthreads();
    const int lim = min(GASS_CT, ncell - base);
    for (int e = wave; e < lim; e += GASS_THREADS / WAVE) {
      const double d0 = e0s[e], d1 = e1s[e];
      const int code = cds[e];
      double p0 = fma(c0, d0, s0 * d1), p1 = fma(c1, d0, s1 * d1);
      if constexpr (EP) { p0 += ems[e]; p1 += ems[e]; }
      acc0 += bern_term(p0, code);
      if (two) acc1 += bern_term(p1, code);
    }
  }
  red[wave][lane] = acc0;
  red[wave][lane + 64] = acc1;
  __syncthreads();
  if (tid < GASS_MAXC) {
    double s = 0.0;
    for (int w = 0; w < GASS_THREADS / WAVE; ++w) s += red[w][tid];
    if (current) { if (tid == 0) a.cur[ch] = s; }
    else if constexpr (ROWS) { if (tid < nth) a.ll[(size_t)ch * GASS_MAXC + tid] += s; }      // (-inf beyond stays)
    else a.ll[(size_t)ch * GASS_MAXC + tid] = tid < nth ? s : -INFINITY;
  }
}
#endif  // BTF_GASS_EP_UNIT

}  // namespace btf
