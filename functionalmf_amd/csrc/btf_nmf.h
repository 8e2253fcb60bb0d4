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
//   [nmf_gram_kernel(V)]  nmf_wpart_kernel  nmf_wsolve_kernel  [nmf_project_kernel]     (fit_W)
//   [nmf_gram_kernel(W)]  nmf_vpart_kernel  nmf_vsolve_kernel  [nmf_project_kernel]  [nmf_pav_kernel]   (fit_V; PAV if monotone)
//   [[nmf_gram_kernel(W)]  nmf_vpart_kernel  nmf_vsolve_kernel  [nmf_project_kernel]]   (row features: the fit of R)
//   nmf_rss_kernel  nmf_decide_kernel
// nmf_project_kernel runs only with max_entry (the reference's SLSQP projection, utils.py:338-347, 369-377, 398-407), the
// third line only with row features; without either the launches and the arithmetic are those of the plain call.
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

constexpr double NMF_XMIN = 1e-6;  // the reference's lower bound on every projected entry (utils.py:345)

enum { NMF_ERR_ITER = 1, NMF_ERR_NONFINITE = 2, NMF_ERR_QP_ITER = 4, NMF_ERR_QP_INFEASIBLE = 8, NMF_ERR_QP_SINGULAR = 16 };

struct NmfState {
  int stop;        // set by nmf_decide_kernel (or an error): the later steps' kernels exit at once
  int steps;       // ALS steps completed
  int err;         // NMF_ERR_* bits
  int err_index;   // a row (W), cell (V, + N) or feature (R, + N + MT) whose NNLS or projection failed
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
  // row features (F = 0: none): every observed x_if joins row i's system as the design row r_f (utils.py:326-329)
  const double* Rf;                          // [F][K]
  const double* SX; const unsigned char* CX; // [N][F]: x_if (0 where missing) and observed (null: all observed)
  int F;
  const unsigned char* skip;                 // V solve: systems left as they are (a feature nobody observed), or null
  int err_base;                              // V solve: err_index of its system 0 (N for cells, N + MT for features)
};

// The feature terms of row i's normal equations, summed over f in order: h_k += x_if r_fk, G_ab += r_fa r_fb (observed f).
__device__ __forceinline__ double nmf_feature_h(const NmfArgs& a, int i, int K, int k, double acc) {
  for (int f = 0; f < a.F; ++f) acc = fma(a.SX[(size_t)i * a.F + f], a.Rf[(size_t)f * K + k], acc);
  return acc;
}
__device__ __forceinline__ double nmf_feature_g(const NmfArgs& a, int i, int K, int p, int b, double acc) {
  for (int f = 0; f < a.F; ++f)
    if (!a.CX || a.CX[(size_t)i * a.F + f]) acc = fma(a.Rf[(size_t)f * K + p], a.Rf[(size_t)f * K + b], acc);
  return acc;
}

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
  if (a.F > 0) {                                         // the terms of nmf_feature_h / nmf_feature_g, one pass over f
    double fh[K], fg[NT];
#pragma unroll
    for (int k = 0; k < K; ++k) fh[k] = sH[k * WAVE + lane];
#pragma unroll
    for (int q = 0; q < NT; ++q) fg[q] = sG[q * WAVE + lane];
    for (int f = 0; f < a.F; ++f) {
      const double xv = a.SX[(size_t)i * a.F + f];
      const bool ob = !a.CX || a.CX[(size_t)i * a.F + f];
      double r[K];
#pragma unroll
      for (int k = 0; k < K; ++k) r[k] = a.Rf[(size_t)f * K + k];
#pragma unroll
      for (int k = 0; k < K; ++k) fh[k] = fma(xv, r[k], fh[k]);
      if (ob) {
#pragma unroll
        for (int p = 0; p < K; ++p)
#pragma unroll
          for (int b = 0; b <= p; ++b) fg[lidx(p, b)] = fma(r[p], r[b], fg[lidx(p, b)]);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) sH[k * WAVE + lane] = fh[k];
#pragma unroll
    for (int q = 0; q < NT; ++q) sG[q * WAVE + lane] = fg[q];
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
  if (c >= a.MT || (a.skip && a.skip[c])) return;
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
  if (it < 0 || !finite) { nmf_fail(a.st, it < 0 ? NMF_ERR_ITER : NMF_ERR_NONFINITE, a.err_base + c); return; }
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
      if (tid < K) nv = pav_merge(w0, sv[t * K + tid], w1, sv[(t + 1) * K + tid]);      // (no product fused into the sum)
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

// ---------------------------------------------------------------- bound check and projection (max_entry)
// The reference (utils.py:338-347, 369-377, 398-407) replaces a fitted system whose entries overshoot max_entry,
//   max_q c_q . x > max_entry   (x = the clipped NNLS solution; only the upper side is looked at),
// by SLSQP's solution of the convex QP
//   min 1/2 |b - A x|^2   subject to   0 <= c_q . x <= max_entry for every q,   x >= 1e-6.
// The rows c_q are shared by all systems of a half-step: all M*T vectors v_jt (leading d entries) for a row of W, all N
// rows of W for a cell of V or a feature row of R.  Here: one wave per system.  The lanes stride over the shared rows
// for the check (a butterfly max); a wave whose system passes leaves at once.  The others solve the QP exactly with
// Goldfarb and Idnani's dual active-set method (Math. Programming 27, 1983) on the normal equations G = A'A, h = A'b,
// summed from the partial slabs (or the complete-data Gram times R, plus the feature terms of a row) in the order of
// the NNLS kernels, so the data is not streamed again:
//   x = G^-1 h;  repeat:  p = the most violated constraint n_p . x >= b_p outside the working set (every lane scans its
//   share of the 2 nq + d constraints, butterfly arg-max, ties to the lowest id; none: done);  then with N the working
//   set's normals, y = G^-1 n_p, r = (N'G^-1 N)^-1 N'y, z = y - G^-1 N r:  step x += t z, u -= t r, u_p += t with
//   t = min(t1 = min_{r_a > 0} u_a / r_a,  t2 = (b_p - n_p . x) / (z . n_p));  t = t2: p joins the working set;
//   t = t1: that constraint leaves it and the step repeats;  t = inf: the constraints contradict each other.
// Each step raises the dual objective, so the method ends after finitely many; a cap of 50 (K + 1) steps reports
// BTF_EINVAL like the NNLS cap.  The working-set algebra (at most K constraints: G^-1, the normals' G^-1 images,
// the Cholesky factor of N'G^-1 N, refactored every step) lives in LDS and is done by lane 0; all lanes share the scan.
// Constraint ids: 2 q = upper side of row q, 2 q + 1 = its lower side, 2 nq + k = x_k >= 1e-6.
struct NmfProj {
  double* X;                   // [nsys][K]: the systems' solutions, replaced where projected
  const double* Cq;            // [nq][K]: the shared constraint rows
  const double* part;          // [nslab][NA][nsys]: the partial slabs of the NNLS pass (h, and G with missing data)
  unsigned char* flag;         // [nsys]: 1 = projected in this step
  int* nproj;                  // the step's count of projected systems
  int nsys, nq, nslab;
  int rows;                    // systems are rows of W: d = min(K, s + 1) unknowns and the feature terms
  int err_base;
  double hi;                   // max_entry
};

__device__ __forceinline__ void nmf_argmax_step(double& v, int& id, double ov, int oid) {
  const bool take = ov > v || (ov == v && oid < id);
  v = take ? ov : v;
  id = take ? oid : id;
}

template <int K, bool MISS>
__global__ __launch_bounds__(WAVE) void nmf_project_kernel(NmfArgs a, NmfProj pj) {
  if (a.st->stop) return;
  constexpr int NT = tri(K), NA = K + (MISS ? NT : 0);
  constexpr double EPS = 2.220446049250313e-16;
  __shared__ double sG[K * K], sGi[K * K], sL[K * K], sH[K], sx[K];
  __shared__ double sAy[K * K], sB[K * K], sLb[K * K], sAu[K], sn[K], sy[K], sz[K], sr[K];
  __shared__ int sAid[K], sI[2];                        // sI: working-set size, failure bits
  const int lane = threadIdx.x, s = blockIdx.x;
  if (a.skip && a.skip[s]) return;
  const int d = pj.rows ? min(K, s + 1) : K;
  const double hi = pj.hi;
  double x[K];
#pragma unroll
  for (int k = 0; k < K; ++k) x[k] = k < d ? pj.X[(size_t)s * K + k] : 0.0;

  // ---- the check: max over the shared rows of c_q . x
  double mx = -INFINITY;
#pragma unroll 4
  for (int q = lane; q < pj.nq; q += WAVE) {
    double dot = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) dot = fma(pj.Cq[(size_t)q * K + k], x[k], dot);
    mx = fmax(mx, dot);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, WAVE));
  if (!(mx > hi)) {
    if (lane == 0) pj.flag[s] = 0;
    return;
  }
  if (lane == 0) {
    pj.flag[s] = 1;
    atomicAdd(pj.nproj, 1);
  }

  // ---- G, h of the system: entry e < K is h_e, entry K + lidx(p, b) is G_pb
  for (int e = lane; e < K + NT; e += WAVE) {
    double v = 0.0;
    if (e < K) {
      for (int c = 0; c < pj.nslab; ++c) v += pj.part[((size_t)c * NA + e) * pj.nsys + s];
      if (pj.rows && a.F > 0) v = nmf_feature_h(a, s, K, e, v);
      sH[e] = v;
    } else {
      const int q = e - K;
      int p = 0;
      while (lidx(p + 1, 0) <= q) ++p;
      const int b = q - lidx(p, 0);
      if constexpr (MISS) {
        for (int c = 0; c < pj.nslab; ++c) v += pj.part[((size_t)c * NA + K + q) * pj.nsys + s];
      } else {
        for (int g = 0; g < NMF_GP; ++g) v += a.gpart[g * NT + q];
        v *= (double)a.R;
      }
      if (pj.rows && a.F > 0) v = nmf_feature_g(a, s, K, p, b, v);
      sG[p * K + b] = v;
      sG[b * K + p] = v;
    }
  }
  __syncthreads();

  // ---- the unconstrained minimiser and G^-1 (leading d block)
  if (lane == 0) {
    int bad = 0;
    for (int p = 0; p < d && !bad; ++p)
      for (int b = 0; b <= p; ++b) {
        double v = sG[p * K + b];
        for (int c = 0; c < b; ++c) v = fma(-sL[p * K + c], sL[b * K + c], v);
        if (p == b) {
          if (!(v > 1e-13 * sG[p * K + p])) { bad = NMF_ERR_QP_SINGULAR; break; }
          sL[p * K + p] = sqrt(v);
        } else {
          sL[p * K + b] = v / sL[b * K + b];
        }
      }
    for (int col = 0; col < d && !bad; ++col) {          // column col of G^-1: L L' g = e_col
      for (int p = 0; p < d; ++p) {
        double v = p == col ? 1.0 : 0.0;
        for (int c = 0; c < p; ++c) v = fma(-sL[p * K + c], sy[c], v);
        sy[p] = v / sL[p * K + p];
      }
      for (int p = d - 1; p >= 0; --p) {
        double v = sy[p];
        for (int c = p + 1; c < d; ++c) v = fma(-sL[c * K + p], sGi[c * K + col], v);
        sGi[p * K + col] = v / sL[p * K + p];
      }
    }
    if (!bad)
      for (int p = 0; p < K; ++p) {
        double v = 0.0;
        if (p < d)
          for (int c = 0; c < d; ++c) v = fma(sGi[p * K + c], sH[c], v);
        sx[p] = v;
      }
    sI[0] = 0;
    sI[1] = bad;
  }

  const int cap = 50 * (K + 1);
  int moves = 0;
  for (;;) {
    __syncthreads();
    if (sI[1]) {
      if (lane == 0) nmf_fail(a.st, sI[1], pj.err_base + s);
      return;
    }
    const int nact = sI[0];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = sx[k];
    // ---- the most violated constraint outside the working set
    double best = 0.0;
    int bid = 0x7fffffff;
    for (int q = lane; q < pj.nq; q += WAVE) {
      double dot = 0.0, sc = hi;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double c = k < d ? pj.Cq[(size_t)q * K + k] : 0.0;
        dot = fma(c, x[k], dot);
        sc = fma(fabs(c), fabs(x[k]), sc);
      }
      const double up = dot - hi;
      const double v = up > 0.0 ? up : -dot;             // at most one side is violated
      const int id = 2 * q + (up > 0.0 ? 0 : 1);
      if (v > 64.0 * EPS * sc) {
        bool in = false;
        for (int w = 0; w < nact; ++w) in = in || sAid[w] == id;
        if (!in) nmf_argmax_step(best, bid, v, id);
      }
    }
    if (lane < d) {
      const double xk = sx[lane], v = NMF_XMIN - xk;
      const int id = 2 * pj.nq + lane;
      if (v > 64.0 * EPS * (fabs(xk) + NMF_XMIN)) {
        bool in = false;
        for (int w = 0; w < nact; ++w) in = in || sAid[w] == id;
        if (!in) nmf_argmax_step(best, bid, v, id);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(best, off, WAVE);
      const int oid = __shfl_xor(bid, off, WAVE);
      nmf_argmax_step(best, bid, ov, oid);
    }
    if (bid == 0x7fffffff) break;                           // feasible: x is the minimiser
    __syncthreads();                                     // every lane has read sx and the working set
    if (lane == 0) {
      // the constraint as n . x >= b0
      double b0;
      if (bid >= 2 * pj.nq) {
        for (int k = 0; k < K; ++k) sn[k] = (k == bid - 2 * pj.nq) ? 1.0 : 0.0;
        b0 = NMF_XMIN;
      } else {
        const double sg = (bid & 1) ? 1.0 : -1.0;
        for (int k = 0; k < K; ++k) sn[k] = k < d ? sg * pj.Cq[(size_t)(bid >> 1) * K + k] : 0.0;
        b0 = (bid & 1) ? 0.0 : -hi;
      }
      int na = nact, bad = 0;
      double uplus = 0.0;
      for (int k = 0; k < d; ++k) {
        double v = 0.0;
        for (int c = 0; c < d; ++c) v = fma(sGi[k * K + c], sn[c], v);
        sy[k] = v;
      }
      double yn = 0.0;
      for (int k = 0; k < d; ++k) yn = fma(sy[k], sn[k], yn);
      for (;;) {
        if (++moves > cap) { bad = NMF_ERR_QP_ITER; break; }
        // r = (N'G^-1 N)^-1 N'y by a Cholesky factorisation of B = N'G^-1 N (na x na)
        for (int p = 0; p < na && !bad; ++p)
          for (int b = 0; b <= p; ++b) {
            double v = sB[p * K + b];
            for (int c = 0; c < b; ++c) v = fma(-sLb[p * K + c], sLb[b * K + c], v);
            if (p == b) {
              if (!(v > 0.0)) { bad = NMF_ERR_QP_SINGULAR; break; }
              sLb[p * K + p] = sqrt(v);
            } else {
              sLb[p * K + b] = v / sLb[b * K + b];
            }
          }
        if (bad) break;
        for (int p = 0; p < na; ++p) {
          double v = 0.0;
          for (int k = 0; k < d; ++k) v = fma(sAy[p * K + k], sn[k], v);
          for (int c = 0; c < p; ++c) v = fma(-sLb[p * K + c], sr[c], v);
          sr[p] = v / sLb[p * K + p];
        }
        for (int p = na - 1; p >= 0; --p) {
          double v = sr[p];
          for (int c = p + 1; c < na; ++c) v = fma(-sLb[c * K + p], sr[c], v);
          sr[p] = v / sLb[p * K + p];
        }
        double zn = 0.0, sp = -b0;
        for (int k = 0; k < d; ++k) {
          double v = sy[k];
          for (int p = 0; p < na; ++p) v = fma(-sr[p], sAy[p * K + k], v);
          sz[k] = v;
          zn = fma(v, sn[k], zn);
          sp = fma(sn[k], sx[k], sp);
        }
        const bool moves_x = na < d && zn > 1e-11 * yn;  // n_p is not spanned by the working set
        const double t2 = moves_x ? fmax(-sp, 0.0) / zn : INFINITY;
        double t1 = INFINITY;
        int l = -1;
        for (int p = 0; p < na; ++p)
          if (sr[p] > 0.0) {
            const double t = sAu[p] / sr[p];
            if (t < t1) { t1 = t; l = p; }
          }
        const double t = fmin(t1, t2);
        if (!(t < INFINITY)) { bad = NMF_ERR_QP_INFEASIBLE; break; }
        for (int p = 0; p < na; ++p) sAu[p] = fmax(fma(-t, sr[p], sAu[p]), 0.0);
        uplus += t;
        if (moves_x)
          for (int k = 0; k < d; ++k) sx[k] = fma(t, sz[k], sx[k]);
        if (t2 <= t1) {                                  // a full step: p joins the working set
          for (int p = 0; p < na; ++p) {
            double v = 0.0;
            for (int k = 0; k < d; ++k) v = fma(sAy[p * K + k], sn[k], v);
            sB[na * K + p] = v;
            sB[p * K + na] = v;
          }
          sB[na * K + na] = yn;
          for (int k = 0; k < K; ++k) sAy[na * K + k] = k < d ? sy[k] : 0.0;
          sAu[na] = uplus;
          sAid[na] = bid;
          ++na;
          break;
        }
        // a partial step: working-set member l leaves
        for (int p = l; p + 1 < na; ++p) {
          sAu[p] = sAu[p + 1];
          sAid[p] = sAid[p + 1];
          for (int k = 0; k < K; ++k) sAy[p * K + k] = sAy[(p + 1) * K + k];
        }
        for (int p = 0; p < na; ++p)                     // B without row and column l
          for (int b = 0; b < na; ++b) {
            const int pp = p < l ? p : p + 1, bb = b < l ? b : b + 1;
            if (pp < na && bb < na && (pp != p || bb != b)) sB[p * K + b] = sB[pp * K + bb];
          }
        --na;
      }
      sI[0] = na;
      sI[1] = bad;
    }
  }
  if (lane < d) {
    if (isfinite(sx[lane])) pj.X[(size_t)s * K + lane] = sx[lane];
    else nmf_fail(a.st, NMF_ERR_NONFINITE, pj.err_base + s);
  }
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
