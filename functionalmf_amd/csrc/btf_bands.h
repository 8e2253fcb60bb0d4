// Simultaneous credible bands per curve over the kept samples: sup-t and rank (depth) bands  (counted under BTF_K_CRITERIA)
//
// For kept sample s and curve (i,j), m_s(t) = f(w_i^s . v_jt^s).  A pointwise band holds each m(t) with the nominal
// probability; the bands here hold the WHOLE curve over the used depths with it (functionalmf_amd/bands.py restates both in
// numpy; that module is the definition).  need = ceil(level / 100 * S).
//   supt   center, scale = mean and sd (ddof 1) over s per cell; D_s = max over the used depths with scale > 0 of
//          |m_s - center| / scale (0 without such a depth); crit = the need-th smallest D_s (an order statistic);
//          lower, upper = center -+ crit * scale at every depth; inside = #{s : D_s <= crit} / S.
//   rank   per cell lo_s = #{s' : m_s' < m_s}, hi_s = #{s' : m_s' > m_s}; depth_s = min over the used depths of
//          min(lo_s, hi_s); k = the largest integer with #{s : depth_s >= k} >= need; lower, upper = the k-th and the
//          (S-1-k)-th order statistic (0-based) of every cell; inside = #{s : depth_s >= k} / S and pointwise_inside the same
//          with k_pw = floor((1 - level / 100) / 2 * S).
//
// supt: three launches per chunk of columns, staged through cen / scl[column][depth][row] and vals[column][sample][row]:
//   band_moments_kernel<K,TR>  one workgroup per (64 rows, column, BAND_TB depths), one lane per row.  Wave p sums the samples
//       s = p, p + BAND_PARTS, ... in sample order; the BAND_PARTS partial sums are added in part order (a fixed order,
//       part of the result's definition).  Two passes: the mean, then the squared deviations from it.
//   band_sweep_kernel<K,TR>    func_sweep_kernel's geometry: a wave takes one sample at a time, D_s lives in a register
//       while t advances, center and scale are read lanes along rows (coalesced).  Every (curve, sample) value is
//       computed by one lane alone: the sample slicing and the chunking of the columns cannot change a bit.
//   band_supt_kernel           func_sort_kernel's geometry: the S values of each curve in an LDS row padded with +inf to a
//       power of two, a bitonic network, the need-th value, and the band of the curve's T depths.
// rank: three launches per chunk of columns, staged through dep[column][slice][row][sample] (integers).  A workgroup owns
// (cells consecutive rows, column, one of zb interleaved slices of the depth axis): the slices give a tensor with few
// curves and many depths (50 x 1 x 370) enough workgroups to fill the chip.
//   band_rank_depth_kernel<K,TR>  per used depth of its slice the S values of each curve are formed and sorted as (key,
//       sample index) pairs in LDS; the run of keys equal to a sample's gives its strict counts lo and hi (two binary
//       searches), min-combined into an integer depth[s] row in LDS and stored per slice.
//   band_rank_k_kernel            the minimum over the slices - of integers, so the slicing cannot change it -, the sorted
//       depth row, k and the two shares.
//   band_rank_write_kernel<K,TR>  every depth of its slice: the keys sorted again, the two order statistics.
//   Integers from the first sort on: nothing is summed in floating point.
// A curve's row costs 8 (key) + 4 (sample index) + 4 (depth) bytes per padded sample: BAND_RANK_MAX_S in 64 KiB.
// fp64 throughout, no atomics.
#pragma once
#include "btf_functionals.h"

namespace btf {

enum { BAND_SUPT = 0, BAND_RANK = 1 };
constexpr int BAND_PARTS = 4;                  // waves per moments workgroup = interleaved partial sums per cell (fixed)
constexpr int BAND_TB = 8;                     // depths per moments workgroup
constexpr int BAND_RANK_LDS = 64 * 1024;       // bytes of LDS for the rows of one rank workgroup: two workgroups per CU
constexpr int BAND_RANK_BYTES = 16;            // per padded sample of a curve: key, sample index, depth
constexpr int BAND_RANK_MAX_S = BAND_RANK_LDS / BAND_RANK_BYTES;   // S <= 4096
constexpr int BAND_CELLS = 16;                 // at most this many curves per supt / rank workgroup
static_assert(BAND_RANK_MAX_S >= 4096, "the rank band takes at least 4096 samples");

struct BandArgs {
  const double* W;          // [S][N][K]
  const double* V;          // [S][M][T][K]
  const int* use;           // [T] 1: the band is simultaneous over this depth
  int S, N, M, T;
  int j0, jc;               // this chunk: columns j0 .. j0 + jc - 1
  int need, kpw;            // ceil(level / 100 * S), floor((1 - level / 100) / 2 * S)
  int P, cells;             // padded row length (power of two >= max(S, 2)) and curves per supt / rank workgroup
  double *cen, *scl;        // supt stage [jc][T][N]
  double* vals;             // supt stage [jc][S][N]
  int zb; int* dep;         // rank stage [jc][zb][N][S]: the depths over each of the zb slices of the depth axis
  const int* curves; int ncurves; double* stat;    // rank: (i,j) pairs and their depth rows [ncurves][S]
  // outputs: center, scale, lower, upper [N][M][T]; crit (supt: crit, rank: k), inside, pw_inside [N][M]
  double *center, *scale, *lower, *upper, *crit, *inside, *pw_inside;
};

using BandKernel = void (*)(BandArgs);
BandKernel band_moments_fn(int K, int transform);    // null outside K = 1..10, transform = 0..2
BandKernel band_sweep_fn(int K, int transform);
BandKernel band_rank_depth_fn(int K, int transform);
BandKernel band_rank_write_fn(int K, int transform);
BandKernel band_supt_fn();
BandKernel band_rank_k_fn();

#ifdef BTF_FUNC_UNIT
template <int K, int TR>
__global__ __launch_bounds__(BAND_PARTS * WAVE) void band_moments_kernel(BandArgs a) {
  __shared__ double part[BAND_PARTS][BAND_TB][WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int jl = blockIdx.y, j = a.j0 + jl;
  const int i = blockIdx.x * WAVE + lane;
  const int ic = i < a.N ? i : a.N - 1;                // clamped row for the loads of the lanes past the end
  const int N = a.N, M = a.M, T = a.T, S = a.S;
  const int t0 = blockIdx.z * BAND_TB, nt = min(BAND_TB, T - t0);
  double mean[BAND_TB] = {};
  for (int pass = 0; pass < 2; ++pass) {
    double sum[BAND_TB];
#pragma unroll
    for (int tt = 0; tt < BAND_TB; ++tt) sum[tt] = 0.0;
    for (int s = wv; s < S; s += BAND_PARTS) {
      const double* __restrict__ wp = a.W + ((size_t)s * N + ic) * K;
      const double* __restrict__ vp = a.V + (((size_t)s * M + j) * T + t0) * K;
      double w[K];
#pragma unroll
      for (int k = 0; k < K; ++k) w[k] = wp[k];
#pragma unroll
      for (int tt = 0; tt < BAND_TB; ++tt) {
        if (tt < nt) {
          double eta = 0.0;
#pragma unroll
          for (int k = 0; k < K; ++k) eta = fma(w[k], vp[tt * K + k], eta);
          const double m = func_transform<TR>(eta);
          if (pass == 0) sum[tt] += m;
          else { const double d = m - mean[tt]; sum[tt] = fma(d, d, sum[tt]); }
        }
      }
    }
    if (pass == 1) __syncthreads();                    // every wave has read the first pass's parts
#pragma unroll
    for (int tt = 0; tt < BAND_TB; ++tt) part[wv][tt][lane] = sum[tt];
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < BAND_TB; ++tt) {
      double tot = part[0][tt][lane];
#pragma unroll
      for (int p = 1; p < BAND_PARTS; ++p) tot += part[p][tt][lane];
      if (pass == 0) mean[tt] = tot / S;
      else if (wv == 0 && i < N && tt < nt) {
        const size_t o = ((size_t)jl * T + t0 + tt) * N + i;
        a.cen[o] = mean[tt];
        a.scl[o] = sqrt(tot / (S - 1));
      }
    }
  }
}

template <int K, int TR>
__global__ __launch_bounds__(FUNC_WAVES * WAVE) void band_sweep_kernel(BandArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int jl = blockIdx.y, j = a.j0 + jl;
  const int i = blockIdx.x * WAVE + lane;
  const int ic = i < a.N ? i : a.N - 1;
  const int N = a.N, M = a.M, T = a.T, S = a.S;
  const int sstride = gridDim.z * FUNC_WAVES;
  const int* __restrict__ use = a.use;
  const double* __restrict__ cen = a.cen + (size_t)jl * T * N + ic;
  const double* __restrict__ scl = a.scl + (size_t)jl * T * N + ic;
  for (int s = blockIdx.z * FUNC_WAVES + wv; s < S; s += sstride) {
    const double* __restrict__ wp = a.W + ((size_t)s * N + ic) * K;
    const double* __restrict__ vp = a.V + ((size_t)s * M + j) * (size_t)T * K;
    double w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = wp[k];
    double D = 0.0;
    for (int t = 0; t < T; ++t) {
      if (!use[t]) continue;                           // (wave-uniform)
      double eta = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) eta = fma(w[k], vp[(size_t)t * K + k], eta);
      const double m = func_transform<TR>(eta);
      const double sc = scl[(size_t)t * N];
      if (sc > 0.0) D = fmax(D, fabs(m - cen[(size_t)t * N]) / sc);
    }
    if (i < N) a.vals[((size_t)jl * S + s) * N + i] = D;
  }
}

// ascending bitonic sort of the `cells` rows of P keys; PAIRS: the sample indices move with their keys
template <bool PAIRS>
__device__ __forceinline__ void band_sort_rows(double* keys, int* idx, int cells, int P) {
  const int half = P >> 1;
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int e = threadIdx.x; e < cells * half; e += 256) {
        const int c = e / half, pidx = e - c * half;
        const int i1 = ((pidx / jj) * 2 * jj) + (pidx % jj), i2 = i1 + jj;
        double* row = keys + (size_t)c * P;
        const double va = row[i1], vb = row[i2];
        const bool up = (i1 & kk) == 0;
        if ((va > vb) == up) {
          row[i1] = vb; row[i2] = va;
          if constexpr (PAIRS) {
            int* ir = idx + (size_t)c * P;
            const int ia = ir[i1];
            ir[i1] = ir[i2]; ir[i2] = ia;
          }
        }
      }
      __syncthreads();
    }
  }
}

// the number of the first n (sorted) values of row below v / not above v
__device__ __forceinline__ int band_count_below(const double* row, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (row[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}
__device__ __forceinline__ int band_count_not_above(const double* row, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (row[mid] <= v) lo = mid + 1; else hi = mid; }
  return lo;
}

__global__ __launch_bounds__(256) void band_supt_kernel(BandArgs a) {
  extern __shared__ double bsrt[];                // [cells][P]
  __shared__ double ccrit[BAND_CELLS];
  const int cells = a.cells, P = a.P, S = a.S, N = a.N, M = a.M, T = a.T;
  const int i0 = blockIdx.x * cells, jl = blockIdx.y, j = a.j0 + jl;
  const int nc = min(cells, N - i0);
  const double* __restrict__ src = a.vals + (size_t)jl * S * N + i0;
  for (int e = threadIdx.x; e < cells * P; e += 256) {
    const int c = e % cells, sidx = e / cells;
    bsrt[(size_t)c * P + sidx] = (sidx < S && c < nc) ? src[(size_t)sidx * N + c] : __builtin_inf();
  }
  __syncthreads();
  band_sort_rows<false>(bsrt, nullptr, cells, P);
  for (int c = threadIdx.x; c < nc; c += 256) {
    const double* row = bsrt + (size_t)c * P;
    const double crit = row[a.need - 1];
    const size_t o = (size_t)(i0 + c) * M + j;
    ccrit[c] = crit;
    a.crit[o] = crit;
    a.inside[o] = (double)band_count_not_above(row, S, crit) / S;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nc * T; e += 256) {
    const int c = e / T, t = e - c * T;
    const size_t in = ((size_t)jl * T + t) * N + i0 + c, o = ((size_t)(i0 + c) * M + j) * T + t;
    const double cn = a.cen[in], sc = a.scl[in];
    double wd;
    {
#pragma clang fp contract(off)
      wd = ccrit[c] * sc;                         // rounded on its own, as the definition's center -+ crit * scale
    }
    a.center[o] = cn; a.scale[o] = sc;
    a.lower[o] = cn - wd; a.upper[o] = cn + wd;
  }
}

// the S values of every curve of the tile at depth t into the key rows: thread -> (curve c, sample s); the curves of a
// sample share v.  PAIRS: the sample indices beside them
template <int K, int TR, bool PAIRS>
__device__ __forceinline__ void band_form_rows(const BandArgs& a, double* bkey, int* bidx, int i0, int nc, int j, int t) {
  const int cells = a.cells, P = a.P, S = a.S, N = a.N, M = a.M, T = a.T;
  for (int e = threadIdx.x; e < cells * P; e += 256) {
    const int c = e % cells, sidx = e / cells;
    double val = __builtin_inf();
    if (sidx < S && c < nc) {
      const double* __restrict__ wp = a.W + ((size_t)sidx * N + i0 + c) * K;
      const double* __restrict__ vp = a.V + (((size_t)sidx * M + j) * T + t) * K;
      double eta = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) eta = fma(wp[k], vp[k], eta);
      val = func_transform<TR>(eta);
    }
    bkey[(size_t)c * P + sidx] = val;
    if constexpr (PAIRS) bidx[(size_t)c * P + sidx] = sidx;
  }
  __syncthreads();
}

template <int K, int TR>
__global__ __launch_bounds__(256) void band_rank_depth_kernel(BandArgs a) {
  extern __shared__ double bkey[];                // [cells][P] keys, then [cells][P] sample indices, then [cells][P] depths
  const int cells = a.cells, P = a.P, S = a.S, N = a.N, T = a.T;
  int* bidx = reinterpret_cast<int*>(bkey + (size_t)cells * P);
  int* bdep = bidx + (size_t)cells * P;
  const int i0 = blockIdx.x * cells, jl = blockIdx.y, j = a.j0 + jl, z = blockIdx.z, zb = gridDim.z;
  const int nc = min(cells, N - i0);
  const int* __restrict__ use = a.use;
  for (int e = threadIdx.x; e < cells * P; e += 256) bdep[e] = S;      // (no count reaches S: a slice without a used depth)
  __syncthreads();
  for (int t = z; t < T; t += zb) {
    if (!use[t]) continue;                         // (uniform over the workgroup)
    band_form_rows<K, TR, true>(a, bkey, bidx, i0, nc, j, t);
    band_sort_rows<true>(bkey, bidx, cells, P);
    // ---- strict counts from the run of equal keys; each (curve, sample) is one thread's
    for (int e = threadIdx.x; e < nc * S; e += 256) {
      const int c = e / S, p = e - c * S;
      const double* row = bkey + (size_t)c * P;
      const double key = row[p];
      const int d = min(band_count_below(row, S, key), S - band_count_not_above(row, S, key));
      int* dp = bdep + (size_t)c * P + bidx[(size_t)c * P + p];
      *dp = min(*dp, d);
    }
    __syncthreads();
  }
  int* __restrict__ dst = a.dep + (((size_t)jl * zb + z) * N + i0) * S;
  for (int e = threadIdx.x; e < nc * S; e += 256) {
    const int c = e / S, sidx = e - c * S;
    dst[e] = bdep[(size_t)c * P + sidx];
  }
}

__global__ __launch_bounds__(256) void band_rank_k_kernel(BandArgs a) {
  extern __shared__ double bkey[];                // [cells][P]: the depths, exact as doubles
  const int cells = a.cells, P = a.P, S = a.S, N = a.N, M = a.M, zb = a.zb;
  const int i0 = blockIdx.x * cells, jl = blockIdx.y, j = a.j0 + jl;
  const int nc = min(cells, N - i0);
  // ---- the minimum over the depth slices: integers, so the slicing cannot change it
  for (int e = threadIdx.x; e < cells * P; e += 256) {
    const int c = e / P, sidx = e - c * P;
    double val = __builtin_inf();
    if (sidx < S && c < nc) {
      int d = S;
      for (int z = 0; z < zb; ++z) d = min(d, a.dep[(((size_t)jl * zb + z) * N + i0 + c) * S + sidx]);
      val = (double)d;
    }
    bkey[e] = val;
  }
  __syncthreads();
  // ---- the raw depths of the requested curves, in sample order
  for (int q = threadIdx.x / WAVE; q < a.ncurves; q += 256 / WAVE) {
    const int c = a.curves[2 * q] - i0;
    if (a.curves[2 * q + 1] != j || c < 0 || c >= nc) continue;
    for (int s = threadIdx.x & (WAVE - 1); s < S; s += WAVE) a.stat[(size_t)q * S + s] = bkey[(size_t)c * P + s];
  }
  __syncthreads();
  // ---- k from the sorted depths: the need-th largest
  band_sort_rows<false>(bkey, nullptr, cells, P);
  for (int c = threadIdx.x; c < nc; c += 256) {
    const double* row = bkey + (size_t)c * P;
    const double k = row[S - a.need];
    const size_t o = (size_t)(i0 + c) * M + j;
    a.crit[o] = k;
    a.inside[o] = (double)(S - band_count_below(row, S, k)) / S;
    a.pw_inside[o] = (double)(S - band_count_below(row, S, (double)a.kpw)) / S;
  }
}

template <int K, int TR>
__global__ __launch_bounds__(256) void band_rank_write_kernel(BandArgs a) {
  extern __shared__ double bkey[];                // [cells][P]
  __shared__ int ck[BAND_CELLS];
  const int cells = a.cells, P = a.P, S = a.S, N = a.N, M = a.M, T = a.T;
  const int i0 = blockIdx.x * cells, j = a.j0 + blockIdx.y;
  const int nc = min(cells, N - i0);
  for (int c = threadIdx.x; c < nc; c += 256)     // (a depth is at most (S-1)/2; the clamp keeps bad data in the row)
    ck[c] = (int)fmin(fmax(a.crit[(size_t)(i0 + c) * M + j], 0.0), (double)((S - 1) / 2));
  for (int t = blockIdx.z; t < T; t += gridDim.z) {
    band_form_rows<K, TR, false>(a, bkey, nullptr, i0, nc, j, t);       // (its barrier also publishes ck)
    band_sort_rows<false>(bkey, nullptr, cells, P);
    for (int c = threadIdx.x; c < nc; c += 256) {
      const double* row = bkey + (size_t)c * P;
      const size_t o = ((size_t)(i0 + c) * M + j) * T + t;
      a.lower[o] = row[ck[c]];
      a.upper[o] = row[S - 1 - ck[c]];
    }
    __syncthreads();
  }
}

#endif  // BTF_FUNC_UNIT

}  // namespace btf
