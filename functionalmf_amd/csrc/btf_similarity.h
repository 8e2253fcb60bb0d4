// Posterior similarity: curve-space distances between rows (or columns) and their neighbours  (counted under BTF_K_CRITERIA)
//
// W is identified only up to an invertible K x K map shared with V, so distances between embeddings mean nothing; the
// distance between two entities' fitted SURFACES mu = W V' is invariant.  For kept sample s, entity e has the coordinates
// x_e,t (K numbers at each of TT depths: w_e and TT = 1 along rows, v_e,t and TT = T along columns) and the members it is
// compared over give the K x K metric  Q_s = sum_members y y'  (along rows the v_jt of the chosen columns, along columns
// the w_i of the chosen rows), n = members x TT cells.  Then (functionalmf_amd/similarity.py restates this in numpy; that
// module is the definition)
//   rms     n d2_s(e,f) = sum_t delta_t' Q_s delta_t,  delta_t = x_e,t - x_f,t;   d = sqrt(max(d2, 0))
//           the difference first, then the form as sum_k delta_k (sum_l Q_kl delta_l): identical entities give exactly 0,
//           and negating delta negates every product exactly, so d(e,f) and d(f,e) are the same bits.
//   cosine  d = 1 - c, c = <e,f> / sqrt(|e|^2 |f|^2) clamped to [-1, 1], <e,f> = sum_t x_lo,t' Q_s x_hi,t with lo < hi the
//           two indices (one order for both (e,f) and (f,e): the same bits); c = 0 when the product of the norms is 0.
// The key neighbours are ordered by is d2 for rms (no root decides a tie) and d for cosine; e itself carries nan and ranks
// last.  Staged by tiles of entities with all S samples and all E partners,  stage[partner f][sample s][local entity e]:
// the layout func_sort_kernel reduces (column = f, row = e) and rank_kernel ranks (along = 0, N = the tile, M = E), both
// launched unchanged.
//   sim_metric_kernel<K>     one workgroup of 256 per sample.  Thread p sums the members p, p + 256, ... into K (K + 1) / 2
//       registers (the lower triangle), a butterfly adds the lanes of a wave and the four waves' sums are added in wave
//       order: a fixed order.  Q is stored full and exactly symmetric.  For cosine the workgroup then takes the squared
//       norm of every entity from the Q in LDS, one lane per entity.  LDS: 4 x 55 + 100 doubles = 2.5 KB at K = 10.
//   sim_dist_kernel<K,COS>   one workgroup of 4 waves per (64 entities of the tile, 32 partners, sample slice); one lane
//       per entity, 8 partners per wave.  Per sample the lower triangle of Q sits in registers (wave-uniform loads), the
//       entities' coordinates go through LDS in blocks of SIM_TB depths (coalesced loads, 64 x (SIM_TB K + 1) doubles:
//       21 KB at K = 10), the partner's coordinates are read at wave-uniform addresses, and 8 accumulators per lane run
//       over the depths.  The key of every (e, f, s) is computed by one lane alone: the tile size, the partner blocks and
//       the sample slicing are pure geometry.  Stores with lanes along e, the fastest-moving axis of the stage.
//   sim_root_kernel          the keys to distances in place, after the ranks are taken (rms: the root; the diagonal: 0),
//       and the (S,E,E) distances when asked for - written transposed, which the symmetry allows: lanes along e.
//   sim_pairs_kernel         the staged distances of the requested (e,f) pairs in sample order.
//   sim_finish_kernel        the tile's integer rank sums to fp64 (one division each, as rank_finish_kernel) and the
//       tile's percentiles to their rows of the (.,E,E) outputs; lanes along f.
// Registers (K = 10): sim_dist_kernel keeps 55 metric entries, 10 coordinates, 10 differences and 8 accumulators in fp64;
// no kernel spills or uses scratch memory (tests/test_host_similarity.py holds them to that).  fp64 throughout, no
// floating-point atomics.
#pragma once
#include "btf_device.h"
#include <math.h>

namespace btf {

constexpr int SIM_THREADS = 256;                    // 4 waves
constexpr int SIM_WAVES = SIM_THREADS / WAVE;
constexpr int SIM_PW = 8;                           // partners a wave carries (accumulators per lane)
constexpr int SIM_FBLK = SIM_WAVES * SIM_PW;        // partners per workgroup
constexpr int SIM_TB = 4;                           // depths per LDS block
constexpr int SIM_MAX_E = 4096;                     // = RANK_MAX_L: a neighbour group is sorted in LDS
constexpr int SIM_MAX_NEAREST = 8;                  // = RANK_MAX_TOP

struct SimArgs {
  const double* X;               // [S][E][TT][K]: the entities' coordinates
  const double* Y;               // [S][YN][mt][K]: where the members come from
  const int* over;               // [nover]: the chosen members' indices in 0..YN-1
  int S, E, TT, YN, mt, nmem;    // nmem = nover * mt member vectors
  double ncells;                 // n = nover * T
  double* metric;                // [S][K][K]
  double* norms;                 // [S][E]: squared norms (cosine), else null
  // this tile: entities e0 .. e0 + ne - 1
  int e0, ne;
  double* stage;                 // [E][S][ne]
  double* dist;                  // [S][E][E] or null
  const int* pairs; int P;       // (e,f) rows
  double* pair_values;           // [S][P]
  // finish
  const unsigned long long* A;   // [ne][E]
  const unsigned long long* B;   // [ne][E]
  const unsigned int* C;         // [ntop][ne][E]
  const double* qtmp;            // [nq][ne][E]
  int ntop, nq, rms;
  double *expected, *rank_var, *pnear, *quant;     // (E,E), (E,E), (ntop,E,E), (nq,E,E)
};

using SimKernel = void (*)(SimArgs);
SimKernel sim_metric_fn(int K);                    // null outside K = 1..10
SimKernel sim_dist_fn(int K, bool cosine);
SimKernel sim_root_fn();
SimKernel sim_pairs_fn();
SimKernel sim_finish_fn();

inline size_t sim_dist_lds_bytes(int K) { return (size_t)WAVE * (SIM_TB * K + 1) * sizeof(double); }

#ifdef BTF_SIM_UNIT
// entry (k,l) of the packed lower triangle
__device__ __forceinline__ constexpr int sim_tri(int k, int l) { return k >= l ? k * (k + 1) / 2 + l : l * (l + 1) / 2 + k; }

// acc + x' Q y with Q the packed lower triangle: sum_k x_k (sum_l Q_kl y_l), every sum an fma chain in index order
template <int K>
__device__ __forceinline__ double sim_form(const double (&q)[K * (K + 1) / 2], const double (&x)[K], const double (&y)[K], double acc) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double z = 0.0;
#pragma unroll
    for (int l = 0; l < K; ++l) z = fma(q[sim_tri(k, l)], y[l], z);
    acc = fma(x[k], z, acc);
  }
  return acc;
}

template <int K>
__global__ __launch_bounds__(SIM_THREADS) void sim_metric_kernel(SimArgs a) {
  constexpr int Q = K * (K + 1) / 2;
  __shared__ double part[SIM_WAVES][Q];
  __shared__ double full[K * K];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  const double* __restrict__ Yb = a.Y + (size_t)s * a.YN * a.mt * K;
  double acc[Q];
#pragma unroll
  for (int n = 0; n < Q; ++n) acc[n] = 0.0;
  for (int m = tid; m < a.nmem; m += SIM_THREADS) {
    const int o = a.over[m / a.mt], r = m % a.mt;
    const double* __restrict__ y = Yb + ((size_t)o * a.mt + r) * K;
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = y[k];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int l = 0; l <= k; ++l) acc[sim_tri(k, l)] = fma(v[k], v[l], acc[sim_tri(k, l)]);
  }
#pragma unroll
  for (int n = 0; n < Q; ++n) {
    const double w = wave_sum(acc[n]);
    if (lane == 0) part[wv][n] = w;
  }
  __syncthreads();
  if (tid < K * K) {
    const int k = tid / K, l = tid - k * K, n = sim_tri(k, l);     // (k,l) and (l,k) add the same parts in the same order
    double sum = 0.0;
    for (int w = 0; w < SIM_WAVES; ++w) sum += part[w][n];
    full[tid] = sum;
    a.metric[(size_t)s * K * K + tid] = sum;
  }
  if (!a.norms) return;
  __syncthreads();
  double q[Q];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int l = 0; l <= k; ++l) q[sim_tri(k, l)] = full[k * K + l];
  for (int e = tid; e < a.E; e += SIM_THREADS) {
    const double* __restrict__ xp = a.X + ((size_t)s * a.E + e) * a.TT * K;
    double nrm = 0.0;
    for (int t = 0; t < a.TT; ++t) {
      double x[K];
#pragma unroll
      for (int k = 0; k < K; ++k) x[k] = xp[(size_t)t * K + k];
      nrm = sim_form<K>(q, x, x, nrm);
    }
    a.norms[(size_t)s * a.E + e] = nrm;
  }
}

template <int K, bool COS>
__global__ __launch_bounds__(SIM_THREADS) void sim_dist_kernel(SimArgs a) {
  constexpr int Q = K * (K + 1) / 2, LS = SIM_TB * K + 1;
  extern __shared__ double sim_x[];                       // [WAVE][LS]: the entities' coordinates of one depth block
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int E = a.E, TT = a.TT, S = a.S, ne = a.ne;
  const int el0 = blockIdx.x * WAVE, el = el0 + lane;     // local entity of the lane
  const bool ok = el < ne;
  const int eg = a.e0 + el;
  const int nb = min(WAVE, ne - el0);                     // entities of this block
  const int f0 = blockIdx.y * SIM_FBLK + wv * SIM_PW;     // this wave's partners f0 .. f0 + SIM_PW - 1
  for (int s = blockIdx.z; s < S; s += gridDim.z) {
    const double* __restrict__ qp = a.metric + (size_t)s * K * K;
    double q[Q];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int l = 0; l <= k; ++l) q[sim_tri(k, l)] = qp[k * K + l];
    const double* __restrict__ Xs = a.X + (size_t)s * E * TT * K;
    double acc[SIM_PW];
#pragma unroll
    for (int p = 0; p < SIM_PW; ++p) acc[p] = 0.0;
    for (int t0 = 0; t0 < TT; t0 += SIM_TB) {
      const int tb = min(SIM_TB, TT - t0), run = tb * K;  // doubles of one entity in this block: contiguous
      __syncthreads();                                    // (the previous block has been read)
      for (int i = tid; i < nb * run; i += SIM_THREADS) {
        const int c = i / run, r = i - c * run;
        sim_x[c * LS + r] = Xs[((size_t)(a.e0 + el0 + c) * TT + t0) * K + r];
      }
      __syncthreads();
      for (int tt = 0; tt < tb; ++tt) {
        double x[K];
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = ok ? sim_x[lane * LS + tt * K + k] : 0.0;
#pragma unroll
        for (int p = 0; p < SIM_PW; ++p) {
          const int f = f0 + p;
          if (f < E) {                                    // (wave-uniform)
            const double* __restrict__ yp = Xs + ((size_t)f * TT + t0 + tt) * K;
            if constexpr (COS) {
              const bool swap = eg > f;                   // the smaller index on the left: one order for (e,f) and (f,e)
              double u[K], v[K];
#pragma unroll
              for (int k = 0; k < K; ++k) { const double y = yp[k]; u[k] = swap ? y : x[k]; v[k] = swap ? x[k] : y; }
              acc[p] = sim_form<K>(q, u, v, acc[p]);
            } else {
              double d[K];
#pragma unroll
              for (int k = 0; k < K; ++k) d[k] = x[k] - yp[k];
              acc[p] = sim_form<K>(q, d, d, acc[p]);
            }
          }
        }
      }
    }
    if (ok) {
#pragma unroll
      for (int p = 0; p < SIM_PW; ++p) {
        const int f = f0 + p;
        if (f < E) {
          double key;
          if constexpr (COS) {
            const double nn = a.norms[(size_t)s * E + eg] * a.norms[(size_t)s * E + f];
            const double c = nn > 0.0 ? fmin(fmax(acc[p] / sqrt(nn), -1.0), 1.0) : 0.0;
            key = 1.0 - c;
          } else {
            key = fmax(acc[p], 0.0) / a.ncells;
          }
          a.stage[((size_t)f * S + s) * ne + el] = eg == f ? __builtin_nan("") : key;
        }
      }
    }
  }
}

// keys to distances in place; the (S,E,E) output transposed (d(e,f) = d(f,e) bit for bit), lanes along e
__global__ __launch_bounds__(256) void sim_root_kernel(SimArgs a) {
  const size_t total = (size_t)a.E * a.S * a.ne;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int el = (int)(i % a.ne);
  const size_t r = i / a.ne;
  const int s = (int)(r % a.S), f = (int)(r / a.S);
  const double key = a.stage[i];
  const double d = f == a.e0 + el ? 0.0 : (a.rms ? sqrt(key) : key);
  a.stage[i] = d;
  if (a.dist) a.dist[((size_t)s * a.E + f) * a.E + a.e0 + el] = d;
}

// one workgroup per pair whose e lies in this tile: its staged distances in sample order
__global__ __launch_bounds__(256) void sim_pairs_kernel(SimArgs a) {
  const int p = blockIdx.x, e = a.pairs[2 * p], f = a.pairs[2 * p + 1];
  if (e < a.e0 || e >= a.e0 + a.ne) return;
  for (int s = threadIdx.x; s < a.S; s += 256)
    a.pair_values[(size_t)s * a.P + p] = a.stage[((size_t)f * a.S + s) * a.ne + (e - a.e0)];
}

// the tile's integer rank sums to fp64 and its percentiles to their rows of the (.,E,E) outputs: one thread per (e, f)
__global__ __launch_bounds__(256) void sim_finish_kernel(SimArgs a) {
  const size_t tile = (size_t)a.ne * a.E, EE = (size_t)a.E * a.E;
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= tile) return;
  const size_t g = (size_t)a.e0 * a.E + o;
  const long long S = a.S, A = (long long)a.A[o], B = (long long)a.B[o];
  a.expected[g] = (double)A / (double)S;
  a.rank_var[g] = S > 1 ? (double)(S * B - A * A) / (double)(S * (S - 1)) : 0.0;   // exact integers below 2^53
  for (int k = 0; k < a.ntop; ++k) a.pnear[k * EE + g] = (double)a.C[k * tile + o] / (double)S;
  for (int k = 0; k < a.nq; ++k) a.quant[k * EE + g] = a.qtmp[k * tile + o];
}
#endif  // BTF_SIM_UNIT

}  // namespace btf
