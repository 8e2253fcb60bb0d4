// Non-negative tensor factorisation by alternating non-negative least squares, and the factor PAV projection
//
// Reference: functionalmf.utils.tensor_nmf (utils.py:276-419) and factor_pav (utils.py:218-252), the starting point of
// almost every chain in the reference's examples.  Context-free: the kernels read their own compact statistics and a
// small state of their own (btf_nmf_create / btf_nmf_run / btf_nmf_pav in btf_nmf.hip); no sampler state is touched.
//
// Statistics (functionalmf_amd/nmf.py builds them once per data tensor), rows outermost so that both passes coalesce:
//   S[i][jt] = sum of the observed replicates y_ijtr,  C[i][jt] = their count (u8; absent when every cell has R)
//   ssw      = sum of (y - cell mean)^2 over the observed entries: a constant of the data
// so that every NNLS system of the reference (design rows repeated per replicate, missing entries dropped) has
//   W row i:   A'A = sum_jt C_ijt v_jt v_jt'   A'b = sum_jt S_ijt v_jt        (leading d = min(K, i+1) block)
//   V cell jt: A'A = sum_i  C_ijt w_i w_i'     A'b = sum_i  S_ijt w_i
// and the residual sum of squares is RSS = ssw + sum_cells (S - C m)^2 / C, m = w_i . v_jt (no cancellation of
// sum y^2 - 2 m S + C m^2).  With complete data the Gram is R times one K x K Gram of the fixed factor (nmf_gram_kernel).
//
// One ALS step, all kernels on one stream, none of them followed by a host synchronisation:
//   [nmf_gram_kernel(V)]  nmf_wpart_kernel  nmf_wsolve_kernel     (fit_W)
//   [nmf_gram_kernel(W)]  nmf_vpart_kernel  nmf_vsolve_kernel  [nmf_pav_kernel]   (fit_V; PAV if monotone)
//   nmf_rss_kernel  nmf_decide_kernel
// nmf_decide_kernel records rmse = sqrt(RSS) and sets the stop flag when (prev - rmse) / rmse <= tol; every kernel of the
// later steps reads the flag first and exits, so W and V stay those of the step that stopped.  Every sum runs in a fixed
// order (per-lane partials in a fixed stride, butterfly wave sums, partial slabs summed in slab order), no floating-point
// atomics: two identical calls give identical bits.
#pragma once
#include "btf_device.h"
#include <math.h>

namespace btf {

constexpr int NMF_MAX_K = 10;
constexpr int NMF_WCH = 1024;      // cells per W-pass workgroup (one wave strides over them)
constexpr int NMF_GP = 64;         // workgroups (partial Grams) of nmf_gram_kernel
constexpr double NMF_FLOOR = 1e-3; // the reference clips every fitted entry to at least this

enum { NMF_ERR_ITER = 1, NMF_ERR_NONFINITE = 2 };

struct NmfState {
  int stop;        // set by nmf_decide_kernel (or an error): the later steps' kernels exit at once
  int steps;       // ALS steps completed
  int err;         // NMF_ERR_* bits
  int err_index;   // a row (W) or cell (V, + N) whose NNLS failed
  double prev;     // the previous step's rmse (inf before the first)
  double delta;    // the last step's (prev - rmse) / rmse
};

struct NmfArgs {
  const double* S; const unsigned char* C;   // [N][MT]; C null: complete data (every count R)
  double* W; double* V;                      // [N][K], [MT][K]
  double* partW;                             // [nchW][NA][N]
  double* partV;                             // [nrcV][NA][MT]
  double* gpart;                             // [NMF_GP][tri(K)]
  double* rpart;                             // [nrss]: nmf_rss_kernel's per-wave partials
  double* hist;                              // [max_steps] rmse per step
  NmfState* st;
  int N, MT, R, nchW, VR, nrcV, nrss;
  double ssw, tol;
};

// ---------------------------------------------------------------- batched NNLS (Lawson-Hanson on the normal equations)
// One lane, one system: G (packed lower triangle, in LDS as G[q * WAVE + lane]) and h = A'b, both K x K / K; only the
// first d variables may become positive.  The passive set P is a bit mask and every loop over the K variables is
// unrolled, so the factor and the vectors stay in registers.  The solve on P is a Cholesky factorisation of G with the
// rows / columns outside P replaced by the identity.  Returns the number of main-loop passes, or -1 when the cap (3d, as
// scipy.optimize.nnls) is reached.
template <int K>
__device__ bool nmf_masked_solve(const double* sG, const double* sH, int lane, unsigned P, double (&s)[K]) {
  double L[tri(K)];
#pragma unroll
  for (int a = 0; a < K; ++a) {
    const bool pa = (P >> a) & 1u;
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      const bool pb = (P >> b) & 1u;
      double v = (pa && pb) ? sG[lidx(a, b) * WAVE + lane] : (a == b ? 1.0 : 0.0);
#pragma unroll
      for (int c = 0; c < b; ++c) v = fma(-L[lidx(a, c)], L[lidx(b, c)], v);
      if (a == b) {
        const double g = (pa ? sG[lidx(a, a) * WAVE + lane] : 1.0);
        if (!(v > 1e-13 * g)) return false;        // not numerically positive definite on P
        L[lidx(a, a)] = sqrt(v);
      } else {
        L[lidx(a, b)] = v / L[lidx(b, b)];
      }
    }
  }
#pragma unroll
  for (int a = 0; a < K; ++a) {
    double v = ((P >> a) & 1u) ? sH[a * WAVE + lane] : 0.0;
#pragma unroll
    for (int c = 0; c < a; ++c) v = fma(-L[lidx(a, c)], s[c], v);
    s[a] = v / L[lidx(a, a)];
  }
#pragma unroll
  for (int a = K - 1; a >= 0; --a) {
    double v = s[a];
#pragma unroll
    for (int c = a + 1; c < K; ++c) v = fma(-L[lidx(c, a)], s[c], v);
    s[a] = v / L[lidx(a, a)];
  }
  return true;
}

template <int K>
__device__ int nmf_nnls(const double* sG, const double* sH, int lane, int d, double (&x)[K]) {
  constexpr double EPS = 2.220446049250313e-16;
  const int cap = 3 * d;
  unsigned P = 0, excl = 0;
  int pass = 0;
#pragma unroll
  for (int a = 0; a < K; ++a) x[a] = 0.0;
  for (;;) {
    // dual w = h - G x; pick the largest w_a > tol over the free, admissible variables
    int jmax = -1;
    double wmax = 0.0;
#pragma unroll
    for (int a = 0; a < K; ++a) {
      double w = sH[a * WAVE + lane], sc = fabs(w);
#pragma unroll
      for (int b = 0; b < K; ++b) {
        const double g = sG[(a >= b ? lidx(a, b) : lidx(b, a)) * WAVE + lane];
        w = fma(-g, x[b], w);
        sc = fma(fabs(g), x[b], sc);
      }
      const bool ok = a < d && !((P >> a) & 1u) && !((excl >> a) & 1u) && w > 16.0 * K * EPS * sc && w > wmax;
      jmax = ok ? a : jmax;
      wmax = ok ? w : wmax;
    }
    if (jmax < 0) return pass;
    if (++pass > cap) return -1;
    P |= 1u << jmax;
    bool first = true;
    for (;;) {
      double s[K];
      if (!nmf_masked_solve<K>(sG, sH, lane, P, s)) {
        if (first) { P &= ~(1u << jmax); excl |= 1u << jmax; break; }   // dependent on P: not admissible this round
        return -1;
      }
      double sj = 0.0;
      bool allpos = true;
#pragma unroll
      for (int a = 0; a < K; ++a) {
        if (a == jmax) sj = s[a];
        if (((P >> a) & 1u) && !(s[a] > 0.0)) allpos = false;
      }
      if (first && !(sj > 0.0)) { P &= ~(1u << jmax); excl |= 1u << jmax; break; }   // Lawson-Hanson's safeguard
      if (allpos) {
#pragma unroll
        for (int a = 0; a < K; ++a) x[a] = ((P >> a) & 1u) ? s[a] : 0.0;
        excl = 0;
        break;
      }
      if (++pass > cap) return -1;
      // step from x toward s until the first passive variable reaches zero, then drop the ones at zero
      double alpha = 2.0;
      int q = -1;
#pragma unroll
      for (int a = 0; a < K; ++a) {
        if (((P >> a) & 1u) && !(s[a] > 0.0)) {
          const double t = x[a] / (x[a] - s[a]);
          if (t < alpha) { alpha = t; q = a; }
        }
      }
#pragma unroll
      for (int a = 0; a < K; ++a) {
        if ((P >> a) & 1u) {
          const double v = fma(alpha, s[a] - x[a], x[a]);
          const bool drop = a == q || !(v > 0.0);
          x[a] = drop ? 0.0 : v;
          if (drop) P &= ~(1u << a);
        }
      }
      first = false;
    }
  }
}

// ---------------------------------------------------------------- Gram of the fixed factor (complete data)
// gpart[g][tri] = sum over rows [g n / GP, (g+1) n / GP) of x x' (lane-strided, butterfly, waves in order)
template <int K>
__global__ __launch_bounds__(256) void nmf_gram_kernel(const double* __restrict__ X, int n, double* __restrict__ gpart,
                                                       const NmfState* st) {
  if (st && st->stop) return;
  constexpr int NT = tri(K);
  __shared__ double red[4][NT];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  const int r0 = (int)((long long)blockIdx.x * n / NMF_GP), r1 = (int)((long long)(blockIdx.x + 1) * n / NMF_GP);
  double acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = 0.0;
  for (int r = r0 + tid; r < r1; r += 256) {
    double x[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = X[(size_t)r * K + k];
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) acc[lidx(a, b)] = fma(x[a], x[b], acc[lidx(a, b)]);
  }
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const double v = wave_sum(acc[q]);
    if (lane == 0) red[wv][q] = v;
  }
  __syncthreads();
  if (tid < NT) gpart[(size_t)blockIdx.x * NT + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// ---------------------------------------------------------------- W pass: right-hand sides (and per-row Grams)
// One wave per (RB rows, NMF_WCH cells); lanes stride over the cells.  partW[chunk][q][i], q < K: sum S v_k;
// q = K + tri (missing data): sum C v_a v_b.
template <int K, int RB, bool MISS>
__global__ __launch_bounds__(WAVE) void nmf_wpart_kernel(NmfArgs a) {
  if (a.st->stop) return;
  constexpr int NA = K + (MISS ? tri(K) : 0);
  const int lane = threadIdx.x;
  const int i0 = blockIdx.x * RB, ch = blockIdx.y;
  const int c0 = ch * NMF_WCH, c1 = min(c0 + NMF_WCH, a.MT);
  double acc[RB][NA];
#pragma unroll
  for (int r = 0; r < RB; ++r)
#pragma unroll
    for (int q = 0; q < NA; ++q) acc[r][q] = 0.0;
  for (int c = c0 + lane; c < c1; c += WAVE) {
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = a.V[(size_t)c * K + k];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      if (i0 + r < a.N) {
        const size_t o = (size_t)(i0 + r) * a.MT + c;
        const double s = a.S[o];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[r][k] = fma(s, v[k], acc[r][k]);
        if constexpr (MISS) {
          const double cn = (double)a.C[o];
#pragma unroll
          for (int p = 0; p < K; ++p) {
            const double cv = cn * v[p];
#pragma unroll
            for (int b = 0; b <= p; ++b) acc[r][K + lidx(p, b)] = fma(cv, v[b], acc[r][K + lidx(p, b)]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if (i0 + r >= a.N) break;
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      const double v = wave_sum(acc[r][q]);
      if (lane == 0) a.partW[((size_t)ch * NA + q) * a.N + i0 + r] = v;
    }
  }
}

// error report of one failed system (racy plain stores of the same kind of value: any one index is kept)
__device__ __forceinline__ void nmf_fail(NmfState* st, int bits, int index) {
  atomicOr(&st->err, bits);
  st->err_index = index;
}

// ---------------------------------------------------------------- W solve: one lane per row
template <int K, bool MISS>
__global__ __launch_bounds__(WAVE) void nmf_wsolve_kernel(NmfArgs a) {
  if (a.st->stop) return;
  constexpr int NT = tri(K), NA = K + (MISS ? NT : 0);
  __shared__ double sG[NT * WAVE], sH[K * WAVE];
  const int lane = threadIdx.x, i = blockIdx.x * WAVE + lane;
  if (i >= a.N) return;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double h = 0.0;
    for (int c = 0; c < a.nchW; ++c) h += a.partW[((size_t)c * NA + k) * a.N + i];
    sH[k * WAVE + lane] = h;
  }
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    double g = 0.0;
    if constexpr (MISS) {
      for (int c = 0; c < a.nchW; ++c) g += a.partW[((size_t)c * NA + K + q) * a.N + i];
    } else {
      for (int p = 0; p < NMF_GP; ++p) g += a.gpart[p * NT + q];
      g *= (double)a.R;
    }
    sG[q * WAVE + lane] = g;
  }
  const int d = min(K, i + 1);
  double x[K];
  const int it = nmf_nnls<K>(sG, sH, lane, d, x);
  bool finite = true;
#pragma unroll
  for (int k = 0; k < K; ++k) finite = finite && isfinite(x[k]);
  if (it < 0 || !finite) { nmf_fail(a.st, it < 0 ? NMF_ERR_ITER : NMF_ERR_NONFINITE, i); return; }
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (k < d) a.W[(size_t)i * K + k] = fmax(x[k], NMF_FLOOR);
}

// ---------------------------------------------------------------- V pass: one lane per cell, one wave per (64 cells, VR rows)
// partV[rc][q][jt], q < K: sum_i S w_ik; q = K + tri (missing data): sum_i C w_a w_b.  w_i is wave-uniform.
template <int K, bool MISS>
__global__ __launch_bounds__(WAVE) void nmf_vpart_kernel(NmfArgs a) {
  if (a.st->stop) return;
  constexpr int NA = K + (MISS ? tri(K) : 0);
  const int lane = threadIdx.x, rc = blockIdx.y;
  const int c = blockIdx.x * WAVE + lane, cc = min(c, a.MT - 1);
  const int r0 = rc * a.VR, r1 = min(r0 + a.VR, a.N);
  double acc[NA];
#pragma unroll
  for (int q = 0; q < NA; ++q) acc[q] = 0.0;
  for (int i = r0; i < r1; ++i) {
    double w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = a.W[(size_t)i * K + k];
    const size_t o = (size_t)i * a.MT + cc;
    const double s = a.S[o];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = fma(s, w[k], acc[k]);
    if constexpr (MISS) {
      const double cn = (double)a.C[o];
#pragma unroll
      for (int p = 0; p < K; ++p) {
        const double cw = cn * w[p];
#pragma unroll
        for (int b = 0; b <= p; ++b) acc[K + lidx(p, b)] = fma(cw, w[b], acc[K + lidx(p, b)]);
      }
    }
  }
  if (c < a.MT) {
#pragma unroll
    for (int q = 0; q < NA; ++q) a.partV[((size_t)rc * NA + q) * a.MT + c] = acc[q];
  }
}

// ---------------------------------------------------------------- V solve: one lane per cell (j, t)
template <int K, bool MISS>
__global__ __launch_bounds__(WAVE) void nmf_vsolve_kernel(NmfArgs a) {
  if (a.st->stop) return;
  constexpr int NT = tri(K), NA = K + (MISS ? NT : 0);
  __shared__ double sG[NT * WAVE], sH[K * WAVE];
  const int lane = threadIdx.x, c = blockIdx.x * WAVE + lane;
  if (c >= a.MT) return;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double h = 0.0;
    for (int r = 0; r < a.nrcV; ++r) h += a.partV[((size_t)r * NA + k) * a.MT + c];
    sH[k * WAVE + lane] = h;
  }
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    double g = 0.0;
    if constexpr (MISS) {
      for (int r = 0; r < a.nrcV; ++r) g += a.partV[((size_t)r * NA + K + q) * a.MT + c];
    } else {
      for (int p = 0; p < NMF_GP; ++p) g += a.gpart[p * NT + q];
      g *= (double)a.R;
    }
    sG[q * WAVE + lane] = g;
  }
  double x[K];
  const int it = nmf_nnls<K>(sG, sH, lane, K, x);
  bool finite = true;
#pragma unroll
  for (int k = 0; k < K; ++k) finite = finite && isfinite(x[k]);
  if (it < 0 || !finite) { nmf_fail(a.st, it < 0 ? NMF_ERR_ITER : NMF_ERR_NONFINITE, a.N + c); return; }
#pragma unroll
  for (int k = 0; k < K; ++k) a.V[(size_t)c * K + k] = fmax(x[k], NMF_FLOOR);
}

// ---------------------------------------------------------------- PAV projection of one column per workgroup
// V[j] (T x K) in LDS.  Pools are runs of depths; pool[t] = first depth of t's pool.  A pass sweeps the pairs (t, t+1)
// left to right; pair t violates if w_i . v_t - w_i . v_{t+1} < 0 for any row i (one block-wide vote).  A violation
// merges t's pool (size w0) and t+1's (size w1) into (w0 v_t + w1 v_{t+1}) / (w0 + w1), in that order per embedding, and
// the sweep continues from the merged pool's last member.  Passes repeat until one merges nothing (every pass but the
// last merges, so there are at most T).  Dynamic LDS: T*K doubles + T ints.
template <int K>
__global__ __launch_bounds__(256) void nmf_pav_kernel(const double* __restrict__ W, double* __restrict__ V, int N, int T,
                                                      const NmfState* st) {
  if (st && st->stop) return;
  extern __shared__ double pav_lds[];
  double* sv = pav_lds;
  int* pool = reinterpret_cast<int*>(pav_lds + (size_t)T * K);
  const int tid = threadIdx.x;
  double* vj = V + (size_t)blockIdx.x * T * K;
  for (int e = tid; e < T * K; e += 256) sv[e] = vj[e];
  for (int t = tid; t < T; t += 256) pool[t] = t;
  __syncthreads();
  for (;;) {
    bool merged = false;
    int t = 0;
    while (t < T - 1) {
      int bad = 0;
      for (int i = tid; i < N; i += 256) {
        double d0 = 0.0, d1 = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const double w = W[(size_t)i * K + k];
          d0 = fma(w, sv[t * K + k], d0);
          d1 = fma(w, sv[(t + 1) * K + k], d1);
        }
        bad |= (d0 - d1 < 0.0);
      }
      if (!__syncthreads_or(bad)) { ++t; continue; }
      const int p0 = pool[t], p1 = pool[t + 1];
      int w0 = 0, w1 = 0, lo = T, hi = -1;
      for (int u = 0; u < T; ++u) {
        const bool in0 = pool[u] == p0, in1 = pool[u] == p1;
        w0 += in0; w1 += in1;
        if (in0 || in1) { lo = min(lo, u); hi = max(hi, u); }
      }
      double nv = 0.0;
      if (tid < K) {
        const double a0 = __dmul_rn((double)w0, sv[t * K + tid]), a1 = __dmul_rn((double)w1, sv[(t + 1) * K + tid]);
        nv = __dadd_rn(a0, a1) / (double)(w0 + w1);
      }
      __syncthreads();                                   // every thread has read the pools and the two depths
      if (tid < K)
        for (int u = lo; u <= hi; ++u) sv[u * K + tid] = nv;
      for (int u = lo + tid; u <= hi; u += 256) pool[u] = p0;
      __syncthreads();
      merged = true;
      t += w1;
    }
    if (!merged) break;
  }
  for (int e = tid; e < T * K; e += 256) vj[e] = sv[e];
}

// ---------------------------------------------------------------- residual sum of squares
// The V pass's geometry: one lane per cell (v_jt in registers), one wave per (64 cells, VR rows), w_i wave-uniform, so a
// cell costs its S (and C) load and K FMAs.  rpart[rc * gridDim.x + block] = the wave's butterfly sum.
template <int K, bool MISS>
__global__ __launch_bounds__(WAVE) void nmf_rss_kernel(NmfArgs a) {
  if (a.st->stop) return;
  const int lane = threadIdx.x, rc = blockIdx.y;
  const int c = blockIdx.x * WAVE + lane, cc = min(c, a.MT - 1);
  const int r0 = rc * a.VR, r1 = min(r0 + a.VR, a.N);
  const double invR = 1.0 / (double)a.R, Rd = (double)a.R;
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = a.V[(size_t)cc * K + k];
  double acc = 0.0;
  for (int i = r0; i < r1; ++i) {
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) m = fma(a.W[(size_t)i * K + k], v[k], m);
    const size_t o = (size_t)i * a.MT + cc;
    const double s = a.S[o];
    if constexpr (MISS) {
      const int cn = a.C[o];
      if (cn > 0) {
        const double r = fma(-(double)cn, m, s);
        acc += r * r / (double)cn;
      }
    } else {
      const double r = fma(-Rd, m, s);
      acc = fma(r * r, invR, acc);
    }
  }
  acc = wave_sum(c < a.MT ? acc : 0.0);
  if (lane == 0) a.rpart[(size_t)rc * gridDim.x + blockIdx.x] = acc;
}

// ---------------------------------------------------------------- the stopping rule, on the device
static __global__ __launch_bounds__(256) void nmf_decide_kernel(NmfArgs a, int step) {
  if (a.st->stop) return;
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  double acc = 0.0;
  for (int p = tid; p < a.nrss; p += 256) acc += a.rpart[p];
  acc = wave_sum(acc);
  if (lane == 0) red[wv] = acc;
  __syncthreads();
  if (tid == 0) {
    const double rss = a.ssw + (((red[0] + red[1]) + red[2]) + red[3]);
    const double rmse = sqrt(rss);
    const double delta = (a.st->prev - rmse) / rmse;
    a.hist[step] = rmse;
    a.st->prev = rmse;
    a.st->delta = delta;
    a.st->steps = step + 1;
    if (delta <= a.tol || a.st->err) a.st->stop = 1;
  }
}

}  // namespace btf
