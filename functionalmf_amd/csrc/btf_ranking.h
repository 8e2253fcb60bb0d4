// Posterior ranking: the rank of every curve within its row or column, per kept sample  (counted under BTF_K_CRITERIA)
//
// For kept sample s and curve (i,j) let f_s(i,j) be one functional of btf_functionals.h.  along = 0 ("cols") ranks the
// M columns within each row (a group is (s, i), L = M members), along = 1 ("rows") the N rows within each column (L = N).
// The rank of a member is 1 + #{members before it} in the order (value, index): ascending or descending in the value,
// ties to the smaller index, nan (an undefined crossing) after every defined value in both orders
// (functionalmf_amd/ranking.py restates this in numpy; that module is the definition).  Per curve, over the samples,
//   A = sum_s r_s,   B = sum_s r_s^2,   C_k = #{s : r_s <= k}     (integers)
//   expected_rank = A / S,   rank_var = (S B - A A) / (S (S - 1)) (0 when S = 1),   p_top[k] = C_k / S
// A property of the JOINT posterior across curves: the curves of one sample are coupled, which no per-curve reduction does.
//
// Staged through a scratch buffer in chunks of SAMPLES (a group needs all its members of one sample at once; the ranks of
// different samples are independent):  vals[column][sample of the chunk][row], written by the unchanged func_sweep_kernel
// (one requested functional, all M columns; the values are bit for bit those of posterior_functionals(pointwise=True)).
//   rank_kernel<ASC>   one workgroup per (tile of G groups, sample slice).  Per sample the tile's values go to LDS as
//       (key, index) pairs, every group padded to the power of two Lp >= L.  The key is the value's bit pattern made
//       monotone as an unsigned integer (sign flip; complemented for the descending order; -0 counts as +0), nan is the
//       largest key and padding the largest key at an index >= L: "nan last" is part of the key, the bitonic network
//       compares (key, index) pairs and has no other branch.  Lanes run along rows when loading, the fastest-moving axis
//       of vals: along = 0 a tile is (G consecutive rows) x (all M columns), along = 1 it is (all N rows) x (G columns).
//       After the sort the member at position p has rank p + 1; the ranks are scattered back to member order, and every
//       thread adds the ranks of the RANK_EPT members it owns into register accumulators over the samples of its slice.
//       At the end they are added to the per-curve 64-bit (A, B) and 32-bit (C_k) integer accumulators with integer
//       atomics: the sums are exact, so neither the order of the additions, the sample slicing nor the chunking can change
//       a bit.  No floating-point atomics.
//   rank_pairs_kernel  for (i,j,i2,j2) pairs anywhere in the tensor: counts of f_s(i,j) < f_s(i2,j2) and of samples in
//       which both are defined, on the raw values func_gather_kernel collects from the chunk.
//   rank_finish_kernel the integers to fp64: one division each.
// LDS of a rank workgroup: G (Lp + 1) 8-byte keys (the +1 spreads the groups of a tile over the banks when lanes run
// along groups) + 2 G Lp 2-byte indices and ranks, G Lp <= 4096: at most 49.7 KB, two workgroups per CU.
#pragma once
#include "btf_device.h"

namespace btf {

constexpr int RANK_MAX_L = 4096;            // members of a group: its padded row must fit one workgroup's LDS
constexpr int RANK_THREADS = 512;
constexpr int RANK_EPT = RANK_MAX_L / RANK_THREADS;   // members a thread owns (register accumulators)
constexpr int RANK_MAX_GROUPS = 64;         // groups per workgroup: a wave of consecutive rows when lanes run along groups
constexpr int RANK_MAX_TOP = 8;

struct RankArgs {
  const double* vals;            // [M][sc][N]: this chunk's values
  int S, N, M;
  int s0, sc;                    // this chunk: samples s0 .. s0 + sc - 1
  int along;                     // 0: rank the columns within a row, 1: the rows within a column
  int L, Lp, lshift, G;          // members of a group, padded (Lp = 1 << lshift), groups per workgroup
  int ntop, top[RANK_MAX_TOP];
  unsigned long long* A;         // [N][M]
  unsigned long long* B;         // [N][M]
  unsigned int* C;               // [ntop][N][M]
  int* ranks;                    // [S][N][M] or null
  // pairs
  int P;
  const double* pvals;           // [2 P][sc]: the raw values of this chunk, (i,j) then (i2,j2) of each pair
  unsigned int* pless;           // [P]
  unsigned int* pdef;            // [P]
  // finish
  double* expected; double* var; double* ptop;   // (N,M), (N,M), (ntop,N,M)
  double* prob_less; double* prob_defined;       // (P,)
};

using RankKernel = void (*)(RankArgs);
RankKernel rank_fn(bool descending);
RankKernel rank_pairs_fn();
RankKernel rank_finish_fn();

// bytes of dynamic LDS of a rank workgroup
inline size_t rank_lds_bytes(int G, int Lp) { return (size_t)G * (Lp + 1) * 8 + (size_t)G * Lp * 4; }

#ifdef BTF_RANK_UNIT
// the sort key of a value: unsigned order = the requested order of the values, nan last in both
template <bool ASC>
__device__ __forceinline__ unsigned long long rank_key(double v) {
  if (v != v) return ~0ull;
  v = v == 0.0 ? 0.0 : v;                                 // -0 == +0: a tie
  unsigned long long b = (unsigned long long)__double_as_longlong(v);
  b = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  return ASC ? b : ~b;                                    // (-inf descending: 0xfff0..., still below nan)
}

template <bool ASC>
__global__ __launch_bounds__(RANK_THREADS) void rank_kernel(RankArgs a) {
  extern __shared__ unsigned long long rk_key[];          // [G][Lp + 1]
  const int Lp = a.Lp, L = a.L, G = a.G, LS = Lp + 1, E = G * Lp, lshift = a.lshift;
  unsigned short* rk_idx = (unsigned short*)(rk_key + (size_t)G * LS);   // [G][Lp]: the member at each sorted position
  unsigned short* rk_rank = rk_idx + E;                                   // [G][Lp]: the rank of each member
  const int N = a.N, M = a.M, sc = a.sc;
  const int g0 = blockIdx.x * G;
  const int ng = min(G, (a.along ? M : N) - g0);          // groups of this tile
  const size_t plane = (size_t)sc * N;                    // vals: doubles per column
  const size_t gstride = a.along ? plane : 1, mstride = a.along ? 1 : plane;
  const int tid = threadIdx.x;

  unsigned int accA[RANK_EPT], accC[RANK_EPT][RANK_MAX_TOP / 2];
  unsigned long long accB[RANK_EPT];
#pragma unroll
  for (int n = 0; n < RANK_EPT; ++n) {
    accA[n] = 0; accB[n] = 0;
#pragma unroll
    for (int k = 0; k < RANK_MAX_TOP / 2; ++k) accC[n][k] = 0;
  }

  for (int s = blockIdx.y; s < sc; s += gridDim.y) {
    const double* __restrict__ src = a.vals + (size_t)s * N + (size_t)g0 * gstride;
    // ---- the (key, index) pairs of the tile: padding first, then the values with lanes along rows
    for (int e = tid; e < E; e += RANK_THREADS) {
      const int g = e >> lshift, m = e & (Lp - 1);
      rk_idx[e] = (unsigned short)m;
      if (m >= L || g >= ng) rk_key[g * LS + m] = ~0ull;
    }
    for (int f = tid; f < ng * L; f += RANK_THREADS) {
      int g, m;
      if (a.along) { g = f / L; m = f - g * L; }          // (all rows) x (a column): rows fastest
      else { m = f / ng; g = f - m * ng; }                // (consecutive rows) x (all columns): rows fastest
      rk_key[g * LS + m] = rank_key<ASC>(src[g * gstride + m * mstride]);
    }
    __syncthreads();
    // ---- bitonic sort of every group on (key, index), ascending
    const int half = Lp >> 1;
    for (int kk = 2; kk <= Lp; kk <<= 1) {
      for (int jj = kk >> 1; jj > 0; jj >>= 1) {
        for (int e = tid; e < (E >> 1); e += RANK_THREADS) {
          const int g = e >> (lshift - 1), p = e & (half - 1);
          if (g < ng) {
            const int i1 = ((p & ~(jj - 1)) << 1) | (p & (jj - 1)), i2 = i1 + jj;
            unsigned long long* kr = rk_key + g * LS;
            unsigned short* ir = rk_idx + (g << lshift);
            const unsigned long long ka = kr[i1], kb = kr[i2];
            const unsigned short ia = ir[i1], ib = ir[i2];
            const bool gt = ka > kb || (ka == kb && ia > ib);
            const bool up = (i1 & kk) == 0;
            if (gt == up) { kr[i1] = kb; kr[i2] = ka; ir[i1] = ib; ir[i2] = ia; }
          }
        }
        __syncthreads();
      }
    }
    // ---- position -> rank of the member
    for (int e = tid; e < E; e += RANK_THREADS) {
      const int g = e >> lshift, p = e & (Lp - 1);
      rk_rank[(g << lshift) + rk_idx[e]] = (unsigned short)(p + 1);
    }
    __syncthreads();
    // ---- every thread adds the ranks of the members it owns
#pragma unroll
    for (int n = 0; n < RANK_EPT; ++n) {
      const int e = tid + n * RANK_THREADS;
      const int g = e >> lshift, m = e & (Lp - 1);
      if (e < E && g < ng && m < L) {
        const unsigned int r = rk_rank[e];
        accA[n] += r;
        accB[n] += (unsigned long long)r * r;
#pragma unroll
        for (int k = 0; k < RANK_MAX_TOP; ++k)
          accC[n][k >> 1] += (r <= (unsigned int)a.top[k] ? 1u : 0u) << (16 * (k & 1));   // two 16-bit counts a register: <= sc <= 8192
        if (a.ranks) {
          const int i = a.along ? m : g0 + g, j = a.along ? g0 + g : m;
          a.ranks[((size_t)(a.s0 + s) * N + i) * M + j] = (int)r;
        }
      }
    }
    // (the next sample's writes of rk_idx / rk_key come after the barrier above; rk_rank is next written after another)
  }
  // ---- into the per-curve integer accumulators
#pragma unroll
  for (int n = 0; n < RANK_EPT; ++n) {
    const int e = tid + n * RANK_THREADS;
    const int g = e >> lshift, m = e & (Lp - 1);
    if (e < E && g < ng && m < L) {
      const int i = a.along ? m : g0 + g, j = a.along ? g0 + g : m;
      const size_t o = (size_t)i * M + j, NM = (size_t)N * M;
      atomicAdd(a.A + o, (unsigned long long)accA[n]);
      atomicAdd(a.B + o, accB[n]);
#pragma unroll
      for (int k = 0; k < RANK_MAX_TOP; ++k)
        if (k < a.ntop) atomicAdd(a.C + k * NM + o, (accC[n][k >> 1] >> (16 * (k & 1))) & 0xffffu);
    }
  }
}

// one workgroup per pair: the samples of this chunk in which f(i,j) < f(i2,j2), and in which both are defined
__global__ __launch_bounds__(256) void rank_pairs_kernel(RankArgs a) {
  __shared__ unsigned int cnt[2][256];
  const int p = blockIdx.x, sc = a.sc;
  const double* __restrict__ va = a.pvals + (size_t)(2 * p) * sc;
  const double* __restrict__ vb = va + sc;
  unsigned int less = 0, def = 0;
  for (int s = threadIdx.x; s < sc; s += 256) {
    const double x = va[s], y = vb[s];
    const bool ok = x == x && y == y;
    def += ok ? 1u : 0u;
    less += (ok && x < y) ? 1u : 0u;
  }
  cnt[0][threadIdx.x] = less; cnt[1][threadIdx.x] = def;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { cnt[0][threadIdx.x] += cnt[0][threadIdx.x + w]; cnt[1][threadIdx.x] += cnt[1][threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { a.pless[p] += cnt[0][0]; a.pdef[p] += cnt[1][0]; }   // one workgroup per pair, chunks in stream order
}

// the integer sums to the fp64 results: one thread per curve, then one per pair
__global__ __launch_bounds__(256) void rank_finish_kernel(RankArgs a) {
  const size_t NM = (size_t)a.N * a.M;
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
  const long long S = a.S;
  if (o < NM) {
    const long long A = (long long)a.A[o], B = (long long)a.B[o];
    if (a.expected) a.expected[o] = (double)A / (double)S;
    if (a.var) a.var[o] = S > 1 ? (double)(S * B - A * A) / (double)(S * (S - 1)) : 0.0;   // exact integers below 2^53
    if (a.ptop)
      for (int k = 0; k < a.ntop; ++k) a.ptop[k * NM + o] = (double)a.C[k * NM + o] / (double)S;
  } else if (o < NM + (size_t)a.P) {
    const size_t p = o - NM;
    a.prob_less[p] = (double)a.pless[p] / (double)S;
    a.prob_defined[p] = (double)a.pdef[p] / (double)S;
  }
}
#endif  // BTF_RANK_UNIT

}  // namespace btf
