// Monotone projection of the posterior: factor_pav of every kept sample's V (counted under BTF_K_CRITERIA)
//
// Reference: doseresponse/fit.py:365-374 projects every kept sample with factor_pav(W_s, V_s[j]) column by column on the
// host (functionalmf/utils.py:218-252), then summarises the projected W V'.  For sample s and column j the projection is
// the left-to-right pool-adjacent-violators sweep of nmf_pav_kernel (btf_nmf.h): pair (t, t+1) violates if
// w_i . v_t - w_i . v_{t+1} < 0 for any row i of W_s; a violation merges t's pool (size w0) and t+1's (size w1) into
// (w0 v_t + w1 v_{t+1}) / (w0 + w1) and the sweep continues at the merged pool's last member; sweeps repeat until one
// merges nothing.  `increasing` is -factor_pav(W_s, -V_s[j]): negation is exact in every step (FMA chain, product, sum,
// quotient), so it is the same sweep with the difference taken the other way round, and the same bits.
// functionalmf_amd/monotone.py (project_host) restates the projection in numpy.
//
//   mono_project_kernel<K>   one workgroup of 256 threads per (column, sample): grid (M, S).  The column's T x K block and
//       one word per depth in LDS (T*K doubles + T ints: the bound of the NMF path's pav_fits, 64 KiB).  The word of depth
//       t holds the first depth of t's pool (low 30 bits) and what is known of the pair (t, t+1) (top 2 bits): unknown,
//       clean (no violation) or violating.  Against nmf_pav_kernel, which serves one W and a chain start:
//       - W_s in registers: thread tid keeps the rows tid, tid + 256, ... (mono_rows(K) of them, K doubles each: 4 rows
//         at K <= 5, 2 at K >= 6) for the whole projection, so N <= 1024 (K <= 5) or N <= 512 (K >= 6) never re-reads W;
//         rows beyond that bound are read from global memory, strided, at every vote (the fallback).
//       - one opening pass votes on every pair at once: a thread walks the depths for its rows, and the projection
//         w_i . v_{t+1} of pair t is pair t+1's w_i . v_t - the same FMA chain (k ascending from 0.0), the same bits.  A
//         thread that sees a violation marks the pair (every writer stores the same word); one barrier ends the pass.  A later vote reuses the projection of its
//         left depth in the same way when the previous vote left it behind.
//       - the sweep then visits the pairs in the reference's order, but votes only where the outcome is not known: a pair
//         whose two depths are unchanged since it voted keeps its outcome, and a pair inside a pool compares two
//         bit-identical rows (difference 0: no violation).  A merge over [lo, hi] changes those depths, so exactly the
//         pairs (lo-1, lo) and (hi, hi+1) become unknown.  The next sweep starts at the first unknown pair, and a sweep
//         that could only find clean pairs is not run: the final empty sweep costs nothing.  A column that is already
//         monotone costs the opening pass (T projections of its rows) and two barriers.
//       The merge arithmetic (pav_merge of btf_device.h: two products, their sum and one division, none of them fused) is
//       nmf_pav_kernel's and numpy's, so the result equals utils.factor_pav and monotone.project_host bit for bit.  Thread 0 writes pools[s][j] = T - merges.  Vout may be Vin (in place): a workgroup
//       reads its block before it writes it, and no other workgroup touches it.
// Build (hipcc -O3, gfx950; -Rpass-analysis=kernel-resource-usage): no instantiation spills or uses scratch.
//   VGPRs  K = 1..5: 48, 62, 76, 90, 104 (4 rows in registers);  K = 6..10: 86, 96, 108, 116, 126 (2 rows)
//   every instantiation allocates at most 128: at least 4 waves per SIMD = four 256-thread workgroups per CU (8 at K = 1,
//   2; 6 at K = 3; 5 at K = 4, 6, 7).  LDS: 256 B static (the block-wide vote) + 8 T K + 4 T dynamic - 2.8 KiB at T = 64,
//   K = 5, 31 KiB at the flu shape's T = 370, K = 10 (five workgroups per CU), 64 KiB at the bound (two).
// fp64, no atomics.
#pragma once
#include "btf_device.h"

namespace btf {

constexpr int MONO_THREADS = 256;
// rows of W a thread keeps in registers (K doubles each): N up to MONO_THREADS * mono_rows(K) never re-reads W
__host__ __device__ constexpr int mono_rows(int K) { return K <= 5 ? 4 : 2; }
constexpr unsigned MONO_CLEAN = 1u << 30, MONO_VIOL = 2u << 30, MONO_START = MONO_CLEAN - 1;   // the word of a depth

struct MonoArgs {
  const double* W;               // [S][N][K]
  const double* Vin;             // [S][M][T][K]
  double* Vout;                  // [S][M][T][K]; may be Vin
  int* pools;                    // [S][M]: T - merges
  int N, M, T, increasing;
};

using MonoKernel = void (*)(MonoArgs);
MonoKernel mono_project_fn(int K);            // null outside K = 1..10

// the column in LDS: the bound of the NMF path's PAV kernel (pav_fits, btf_nmf.hip)
inline size_t mono_lds(int T, int K) { return (size_t)T * K * sizeof(double) + (size_t)T * sizeof(int); }
inline bool mono_fits(int T, int K) { return T < (int)MONO_CLEAN && mono_lds(T, K) <= 64 * 1024; }

#ifdef BTF_MONOTONE_UNIT
template <int K>
__device__ __forceinline__ double mono_dot(const double (&w)[K], const double* v) {
  double d = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) d = fma(w[k], v[k], d);
  return d;
}

__device__ __forceinline__ bool mono_violates(double d0, double d1, bool inc) { return inc ? (d1 - d0 < 0.0) : (d0 - d1 < 0.0); }

template <int K>
__global__ __launch_bounds__(MONO_THREADS) void mono_project_kernel(MonoArgs a) {
  extern __shared__ __attribute__((aligned(16))) double mono_smem[];
  const int tid = threadIdx.x, N = a.N, T = a.T;
  double* sv = mono_smem;
  unsigned* pool = reinterpret_cast<unsigned*>(mono_smem + (size_t)T * K);
  const size_t col = (size_t)blockIdx.y * a.M + blockIdx.x;
  const double* __restrict__ W = a.W + (size_t)blockIdx.y * N * K;
  const double* vin = a.Vin + col * T * K;
  double* vout = a.Vout + col * T * K;
  const bool inc = a.increasing != 0;
  constexpr int MONO_ROWS = mono_rows(K), MONO_RESIDENT = MONO_THREADS * MONO_ROWS;
  const int nr = min(MONO_ROWS, (N + MONO_THREADS - 1) / MONO_THREADS);     // register rows in use (uniform)

  double w[MONO_ROWS][K];
#pragma unroll
  for (int r = 0; r < MONO_ROWS; ++r) {
    const int i = tid + r * MONO_THREADS;
#pragma unroll
    for (int k = 0; k < K; ++k) w[r][k] = i < N ? W[(size_t)i * K + k] : 0.0;     // (a zero row never violates)
  }
  for (int e = tid; e < T * K; e += MONO_THREADS) sv[e] = vin[e];
  for (int t = tid; t < T; t += MONO_THREADS) pool[t] = (unsigned)t | MONO_CLEAN;
  __syncthreads();

  // ---- the opening pass: every pair's vote, the projections chained along depth
  if (T > 1) {
    double d0[MONO_ROWS];
#pragma unroll
    for (int r = 0; r < MONO_ROWS; ++r) d0[r] = r < nr ? mono_dot<K>(w[r], sv) : 0.0;
    for (int t = 0; t < T - 1; ++t) {
      bool bad = false;
#pragma unroll
      for (int r = 0; r < MONO_ROWS; ++r)
        if (r < nr) {
          const double d1 = mono_dot<K>(w[r], sv + (size_t)(t + 1) * K);
          bad |= mono_violates(d0[r], d1, inc);
          d0[r] = d1;
        }
      if (bad) pool[t] = (unsigned)t | MONO_VIOL;            // (every writer stores the same word)
    }
    for (int i = MONO_RESIDENT + tid; i < N; i += MONO_THREADS) {      // rows beyond the registers
      double wi[K];
#pragma unroll
      for (int k = 0; k < K; ++k) wi[k] = W[(size_t)i * K + k];
      double e0 = mono_dot<K>(wi, sv);
      for (int t = 0; t < T - 1; ++t) {
        const double e1 = mono_dot<K>(wi, sv + (size_t)(t + 1) * K);
        if (mono_violates(e0, e1, inc)) pool[t] = (unsigned)t | MONO_VIOL;
        e0 = e1;
      }
    }
  }

  // ---- the sweeps: the reference's order of visits, a vote only where the outcome is not known
  int merges = 0, start = 0, have = -1;        // have: the depth whose projections p[] holds (-1: none)
  double p[MONO_ROWS];
#pragma unroll
  for (int r = 0; r < MONO_ROWS; ++r) p[r] = 0.0;
  while (start < T - 1) {
    __syncthreads();                           // the words and depths the last sweep (or the opening pass) wrote
    int t = start;
    start = T;
    while (t < T - 1) {
      const unsigned word = pool[t], known = word & ~MONO_START;
      if (known == MONO_CLEAN) { ++t; continue; }
      if (known == 0) {                        // unknown: vote
        int bad = 0;
        double d1[MONO_ROWS];
#pragma unroll
        for (int r = 0; r < MONO_ROWS; ++r) {
          d1[r] = 0.0;
          if (r < nr) {
            const double d0 = have == t ? p[r] : mono_dot<K>(w[r], sv + (size_t)t * K);
            d1[r] = mono_dot<K>(w[r], sv + (size_t)(t + 1) * K);
            bad |= mono_violates(d0, d1[r], inc);
          }
        }
        for (int i = MONO_RESIDENT + tid; i < N; i += MONO_THREADS) {
          double wi[K];
#pragma unroll
          for (int k = 0; k < K; ++k) wi[k] = W[(size_t)i * K + k];
          bad |= mono_violates(mono_dot<K>(wi, sv + (size_t)t * K), mono_dot<K>(wi, sv + (size_t)(t + 1) * K), inc);
        }
        if (!__syncthreads_or(bad)) {
#pragma unroll
          for (int r = 0; r < MONO_ROWS; ++r) p[r] = d1[r];
          have = t + 1;
          if (tid == 0) pool[t] = word | MONO_CLEAN;         // read again after the next sweep's opening barrier at the earliest
          ++t;
          continue;
        }
      }
      // merge t's pool [p0, t] and t+1's pool [t+1, hi]
      const int p0 = (int)(word & MONO_START);
      int hi = t + 1;
      while (hi + 1 < T && (int)(pool[hi + 1] & MONO_START) == t + 1) ++hi;
      const int w0 = t + 1 - p0, w1 = hi - t;
      double nv = 0.0;
      if (tid < K) nv = pav_merge(w0, sv[(size_t)t * K + tid], w1, sv[(size_t)(t + 1) * K + tid]);
      __syncthreads();                                     // every thread has read the words and the two depths
      if (tid < K)
        for (int u = p0; u <= hi; ++u) sv[(size_t)u * K + tid] = nv;
      for (int u = t + tid; u <= hi; u += MONO_THREADS) pool[u] = (unsigned)p0 | (u < hi ? MONO_CLEAN : 0u);
      if (p0 > 0) {
        if (tid == 0) pool[p0 - 1] &= MONO_START;          // the pair to the left of the merged pool: unknown again
        start = min(start, p0 - 1);
      }
      __syncthreads();
      ++merges;
      have = -1;
      t = hi;
    }
  }
  if (merges || vout != vin)
    for (int e = tid; e < T * K; e += MONO_THREADS) vout[e] = sv[e];
  if (tid == 0 && a.pools) a.pools[col] = T - merges;
}
#endif  // BTF_MONOTONE_UNIT

}  // namespace btf
