// Posterior curve functionals over the kept samples: AUC, peak, level crossing  (counted under BTF_K_CRITERIA)
//
// Reference: doseresponse/feature_importance.py:40 forms einsum('znk,zmtk->znmt', Ws, Vs) on the host and takes
// np.trapz(., dx=1/(T-1), axis=-1).mean(axis=0).  Here, for kept sample s and curve (i,j), m_t = f(w_i^s . v_jt^s) over
// the depth coordinates x_0 < ... < x_{T-1} is reduced in ONE pass over t to seven numbers (functionalmf_amd/functionals.py
// restates them in numpy; that module is the definition):
//   0 auc       sum_t (x_t - x_{t-1}) (m_t + m_{t-1}) / 2
//   1 max       2 min
//   3 argmax    4 argmin     x at the first occurrence of the extreme
//   5 rise      sum_t max(m_t - m_{t-1}, 0)
//   6 crossing  d = m - level: x_0 if d_0 == 0, else at the first t with d_t d_{t+1} < 0 or d_{t+1} == 0
//               x_t + (x_{t+1} - x_t) d_t / (d_t - d_{t+1}); nan (undefined) when the level is never crossed
// and the S values of every curve and requested functional to mean, variance (ddof 1), percentiles, the share of defined
// samples and the share above a threshold.  The (S,N,M,T) tensor is never formed and no curve is stored.
//
// Two launches per chunk of columns, staged through a scratch buffer  vals[slot][column][sample][row]:
//   func_sweep_kernel<K,TR>  one workgroup per (64 rows, column, sample slice), one lane per row.  A wave takes one sample
//       at a time: w_i^s is K per-lane loads, v_jt^s and x_t are read at wave-uniform addresses (one broadcast load), the seven
//       running functionals live in registers while t advances.  The requested ones are stored, lanes along rows
//       (coalesced).  Every (curve, sample) value is computed by one lane alone, so the sample slicing (gridDim.z) and the
//       chunking of the columns are pure geometry: they cannot change a bit of the result.
//   func_sort_kernel         one workgroup per (FUNC cells consecutive rows, column, requested functional).  The S values of
//       each curve go to an LDS row padded to a power of two with +inf (an undefined crossing counts as +inf:
//       right-censored), a bitonic network sorts the rows, and mean / M2 / counts are summed over the sorted row in
//       FUNC_PARTS interleaved partial sums that are added in part order: a fixed order, independent of the launch.
//       Two-pass variance (mean first, then squared deviations).  Percentiles by numpy's linear rule; one that touches
//       a non-finite order statistic is nan.
// The host keeps a chunk's scratch under FUNC_SCRATCH_BYTES so that it stays in the 256 MiB Infinity Cache between the two
// launches; only the requested functionals are stored and sorted.  fp64 throughout, no atomics.
#pragma once
#include "btf_device.h"
#include <math.h>

namespace btf {

enum { FUNC_AUC = 0, FUNC_MAX = 1, FUNC_MIN = 2, FUNC_ARGMAX = 3, FUNC_ARGMIN = 4, FUNC_RISE = 5, FUNC_CROSSING = 6, FUNC_COUNT = 7 };
constexpr int FUNC_WAVES = 4;                 // waves per sweep workgroup
constexpr int FUNC_SORT_LDS = 64 * 1024;      // bytes of LDS for the rows of one sort workgroup: two workgroups per CU
constexpr int FUNC_MAX_S = FUNC_SORT_LDS / 8; // one curve's padded row of doubles must fit them: S <= 8192
constexpr int FUNC_SORT_CELLS = 16;           // at most this many curves per sort workgroup
constexpr int FUNC_PARTS = 16;                // interleaved partial sums per curve (fixed: part of the result's definition)
constexpr size_t FUNC_SCRATCH_BYTES = (size_t)192 << 20;

struct FuncArgs {
  const double* W;          // [S][N][K]
  const double* V;          // [S][M][T][K]
  const double* x;          // [T] strictly increasing
  double level, exceed;
  int S, N, M, T;
  int j0, jc;               // this chunk: columns j0 .. j0 + jc - 1
  int slot[FUNC_COUNT];     // scratch / output slot of each functional, -1: not requested
  int code[FUNC_COUNT];     // functional of each slot
  int nslots;
  double* vals;             // [nslots][jc][S][N]
  double* pw;               // [nslots][S][N][M] or null
  // sort outputs, (N,M) planes per slot; any may be null
  const double* q; int nq;
  double* mean; double* var; double* quant;   // quant [nslots][nq][N][M]
  double* defined;          // [N][M]: the crossing slot only
  double* prob;             // [nslots][N][M]
  int P, cells;             // padded row length (power of two >= max(S, 2)) and curves per sort workgroup
};

// the kernels live in btf_functionals.hip (a compilation unit of their own); the C-ABI unit launches them through these
using FuncKernel = void (*)(FuncArgs);
using FuncGatherKernel = void (*)(FuncArgs, const int*, int, double*);
FuncKernel func_sweep_fn(int K, int transform);      // null outside K = 1..10, transform = 0..2
FuncKernel func_sort_fn();
FuncGatherKernel func_gather_fn();

#ifdef BTF_FUNC_UNIT
template <int TR>
__device__ __forceinline__ double func_transform(double x) {
  if constexpr (TR == 1) return 1.0 / (1.0 + exp(-x));
  else if constexpr (TR == 2) return x * x;
  else return x;
}

template <int K, int TR>
__global__ __launch_bounds__(FUNC_WAVES * WAVE) void func_sweep_kernel(FuncArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int jl = blockIdx.y, j = a.j0 + jl;
  const int i = blockIdx.x * WAVE + lane;
  const bool row_ok = i < a.N;
  const int ic = row_ok ? i : a.N - 1;                 // clamped row for the loads of the lanes past the end
  const int N = a.N, M = a.M, T = a.T, S = a.S;
  const int sstride = gridDim.z * FUNC_WAVES;
  const double* __restrict__ xs = a.x;
  const double x0 = xs[0];
  for (int s = blockIdx.z * FUNC_WAVES + wv; s < S; s += sstride) {
    const double* __restrict__ wp = a.W + ((size_t)s * N + ic) * K;
    const double* __restrict__ vp = a.V + ((size_t)s * M + j) * (size_t)T * K;
    double w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = wp[k];
    double eta = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) eta = fma(w[k], vp[k], eta);
    double mp = func_transform<TR>(eta), xp = x0;
    double auc = 0.0, rise = 0.0, mx = mp, mn = mp, xmx = x0, xmn = x0;
    double dp = mp - a.level;
    double cross = dp == 0.0 ? x0 : __builtin_nan("");
    bool found = dp == 0.0;
    for (int t = 1; t < T; ++t) {
      eta = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) eta = fma(w[k], vp[(size_t)t * K + k], eta);
      const double m = func_transform<TR>(eta), xt = xs[t], dx = xt - xp;
      auc = fma(0.5 * dx, m + mp, auc);
      rise += fmax(m - mp, 0.0);
      if (m > mx) { mx = m; xmx = xt; }
      if (m < mn) { mn = m; xmn = xt; }
      const double dc = m - a.level;
      if (!found && (dp * dc < 0.0 || dc == 0.0)) { cross = xp + dx * (dp / (dp - dc)); found = true; }
      mp = m; xp = xt; dp = dc;
    }
    if (row_ok) {
      const double out[FUNC_COUNT] = {auc, mx, mn, xmx, xmn, rise, cross};
#pragma unroll
      for (int f = 0; f < FUNC_COUNT; ++f) {
        const int sl = a.slot[f];
        if (sl >= 0) {
          a.vals[(((size_t)sl * a.jc + jl) * S + s) * N + i] = out[f];
          if (a.pw) a.pw[(((size_t)sl * S + s) * N + i) * M + j] = out[f];
        }
      }
    }
  }
}

// the raw values of the requested curves in sample order: out[slot][curve][s]; curves (i, j) pairs
__global__ void func_gather_kernel(FuncArgs a, const int* __restrict__ curves, int ncurves, double* __restrict__ out) {
  const int c = blockIdx.x, sl = blockIdx.y;
  const int i = curves[2 * c], j = curves[2 * c + 1];
  if (j < a.j0 || j >= a.j0 + a.jc) return;
  const int jl = j - a.j0;
  for (int s = threadIdx.x; s < a.S; s += blockDim.x)
    out[((size_t)sl * ncurves + c) * a.S + s] = a.vals[(((size_t)sl * a.jc + jl) * a.S + s) * a.N + i];
}

__global__ __launch_bounds__(256) void func_sort_kernel(FuncArgs a) {
  extern __shared__ double srt[];                 // [cells][P]
  __shared__ double psum[FUNC_SORT_CELLS][FUNC_PARTS];
  __shared__ int pcnt[FUNC_SORT_CELLS][FUNC_PARTS], pabove[FUNC_SORT_CELLS][FUNC_PARTS];
  __shared__ double cmean[FUNC_SORT_CELLS];
  __shared__ int ccnt[FUNC_SORT_CELLS];
  const int cells = a.cells, P = a.P, S = a.S, N = a.N, M = a.M;
  const int i0 = blockIdx.x * cells, jl = blockIdx.y, j = a.j0 + jl, sl = blockIdx.z;
  const int nc = min(cells, N - i0);
  const bool censor = a.code[sl] == FUNC_CROSSING;
  const double* __restrict__ src = a.vals + ((size_t)sl * a.jc + jl) * (size_t)S * N + i0;
  // ---- values: thread -> (curve c, sample s); vals[.][s][i0 + c] is contiguous over c
  for (int e = threadIdx.x; e < cells * P; e += 256) {
    const int c = e % cells, sidx = e / cells;
    double val = __builtin_inf();
    if (sidx < S && c < nc) {
      val = src[(size_t)sidx * N + c];
      if (val != val) val = __builtin_inf();       // undefined crossing: right-censored
    }
    srt[(size_t)c * P + sidx] = val;
  }
  __syncthreads();
  // ---- bitonic sort of every row (ascending), as posterior_summary_kernel
  const int half = P >> 1;
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int e = threadIdx.x; e < cells * half; e += 256) {
        const int c = e / half, pidx = e - c * half;
        const int i1 = ((pidx / jj) * 2 * jj) + (pidx % jj), i2 = i1 + jj;
        double* row = srt + (size_t)c * P;
        const double va = row[i1], vb = row[i2];
        const bool up = (i1 & kk) == 0;
        if ((va > vb) == up) { row[i1] = vb; row[i2] = va; }
      }
      __syncthreads();
    }
  }
  // ---- pass 1: sum, count of defined values and of values above the threshold; part p takes s = p, p + PARTS, ...
  for (int e = threadIdx.x; e < nc * FUNC_PARTS; e += 256) {
    const int c = e / FUNC_PARTS, p = e % FUNC_PARTS;
    const double* row = srt + (size_t)c * P;
    double sum = 0.0;
    int cnt = 0, above = 0;
    for (int sidx = p; sidx < S; sidx += FUNC_PARTS) {
      const double v = row[sidx];
      const bool ok = !censor || v < __builtin_inf();
      if (ok) { sum += v; ++cnt; above += v > a.exceed ? 1 : 0; }
    }
    psum[c][p] = sum; pcnt[c][p] = cnt; pabove[c][p] = above;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nc; c += 256) {
    double sum = 0.0;
    int cnt = 0, above = 0;
    for (int p = 0; p < FUNC_PARTS; ++p) { sum += psum[c][p]; cnt += pcnt[c][p]; above += pabove[c][p]; }
    const size_t o = (size_t)sl * N * M + (size_t)(i0 + c) * M + j;
    const double mean = cnt > 0 ? sum / cnt : __builtin_nan("");
    cmean[c] = mean; ccnt[c] = cnt;
    if (a.mean) a.mean[o] = mean;
    if (a.prob) a.prob[o] = (double)above / S;
    if (a.defined && censor) a.defined[(size_t)(i0 + c) * M + j] = (double)cnt / S;
  }
  __syncthreads();
  // ---- pass 2: squared deviations from the mean, same parts and order
  for (int e = threadIdx.x; e < nc * FUNC_PARTS; e += 256) {
    const int c = e / FUNC_PARTS, p = e % FUNC_PARTS;
    const double* row = srt + (size_t)c * P;
    const double mean = cmean[c];
    double sum = 0.0;
    for (int sidx = p; sidx < S; sidx += FUNC_PARTS) {
      const double v = row[sidx];
      if (!censor || v < __builtin_inf()) { const double d = v - mean; sum = fma(d, d, sum); }
    }
    psum[c][p] = sum;
  }
  __syncthreads();
  if (a.var)
    for (int c = threadIdx.x; c < nc; c += 256) {
      double sum = 0.0;
      for (int p = 0; p < FUNC_PARTS; ++p) sum += psum[c][p];
      a.var[(size_t)sl * N * M + (size_t)(i0 + c) * M + j] = ccnt[c] > 1 ? sum / (ccnt[c] - 1) : __builtin_nan("");
    }
  // ---- percentiles: numpy's default ('linear'); nan where an order statistic it touches is not finite
  for (int e = threadIdx.x; e < nc * a.nq; e += 256) {
    const int c = e % nc, qi = e / nc;
    const double* row = srt + (size_t)c * P;
    const double pos = a.q[qi] * 0.01 * (S - 1);
    int lo = (int)floor(pos);
    lo = max(0, min(lo, S - 1));
    const int hi = min(lo + 1, S - 1);
    const double frac = pos - lo, vl = row[lo], vh = row[hi];
    const bool fin = fabs(vl) < __builtin_inf() && fabs(vh) < __builtin_inf();
    a.quant[(((size_t)sl * a.nq + qi) * N + i0 + c) * M + j] = fin ? vl + frac * (vh - vl) : __builtin_nan("");
  }
}

#endif  // BTF_FUNC_UNIT

}  // namespace btf
