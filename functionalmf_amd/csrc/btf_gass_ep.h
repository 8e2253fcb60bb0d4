// EP-centred proposals of the constrained model's GASS updates (ep_approx; factor.py:677-688 rows, :771-793 columns,
// gass.py:21-41 and :114 the centred ellipse).  With p = 1 / Sigma_ep^2 per cell:
//   row i      Q_i = sum_{j,t} p v_jt v_jt' + I_d / sigma2 over the first d = min(K, i+1) dimensions,
//              mu_i = Q_i^-1 sum_{j,t} p Mu v_jt, proposal L_i'^-1 z (L_i L_i' = Q_i)
//   column j   Q = kron(I_K, Delta' Lambda_j Delta) + X' Sigma X (X = kron(W, I_T)): the per-depth blocks
//              sum_i p w_i w_i' beside the prior band, mu = Q^-1 X' Sigma Mu[:, j], proposal P' L^-T z with L L' = P Q P'
//              for the twisted elimination order the plain GASS prior draw declares
// The GASS passes then run on x0 = x - mu and add mu back; the likelihood of every candidate (and of the current
// state) is corrected by - sum_cells log N(tau; Mu, Sigma_ep) = sum_cells p (tau - Mu)^2 / 2 + log Sigma_ep + log(2 pi) / 2
// (factor.py:727-757, :856-891): in gass_eval_kernel<..., true> the quadratic's sum as a per-chain quadratic form in
// (cos, sin, 1) summed while the cells are staged, the constants per chain from the host (btf_gass_set_ep).
//
//   gass_ep_rows_kernel<K>   one workgroup per row: the statistics (Mu, p) of the row's cells, V from cache; fixed-order
//                            sums (lanes, then a butterfly per wave, then the four waves in order); the d x d solve and
//                            the proposal in thread 0.  Also the current state's correction.
//   gass_ep_cols_kernel<K>   one workgroup per column: per-depth blocks (a wave per depth, lanes over rows), then the
//                            KT x KT system in profile (envelope) storage in the twisted order - a right-looking Cholesky
//                            that stays in the envelope, one forward and two backward substitutions (mean and noise).
//   gass_ep_fix_kernel       cur_ll and the slice height += the current state's correction
//   gass_ep_commit_kernel    x = x0 cos + v sin + mu for the chains the host selected
// Every sum has a fixed order: two calls give identical bits.
#pragma once
#include "btf_device.h"

namespace btf {

constexpr int GEP_THREADS = 256;
constexpr int GEP_MAXK = 10;

struct GassEpArgs {
  const double2* ep;        // rows: [N][M*T] (Mu, p); cols: [M][T][N]
  const double* cconst;     // [nchains] sum of log Sigma_ep + log(2 pi) / 2 over the chain's cells
  const double* W; const double* V;
  int N, M, T, K, TF;
  double sigma2; const double* sigma2_dev;       // rows: the prior variance (device-resident when sigma2_dev)
  const double* pband;      // cols: [M][T][TF+2] the prior band Delta' Lambda_j Delta
  const int* env_f; const int* env_off; int env_size, bwe;    // cols: envelope of P Q P' (first column, offset per row)
  double* env_g;            // cols: envelope scratch in HBM [M][env_size] (nullptr: LDS)
  const double* z; unsigned long long seed, stream;
  double* X0; double* Nu; double* Mu; double* corr;
  int* status;
};

using GassEpKernel = void (*)(GassEpArgs);
using GassEpFixKernel = void (*)(const double*, int, double*, double*);
using GassEpCommitKernel = void (*)(const double*, const double*, const double*, double*, long long, int, const double*, const int*);
// btf_gass_ep.hip: the kernels of this unit by nembeds (nullptr outside 1..GEP_MAXK), for Prof::launch in btf_abi.hip
GassEpKernel gass_ep_rows_fn(int K);
GassEpKernel gass_ep_cols_fn(int K);
GassEpFixKernel gass_ep_fix_fn();
GassEpCommitKernel gass_ep_commit_fn();
// dynamic LDS of gass_ep_cols_kernel: the vectors and blocks, plus the envelope when it is held on chip
inline size_t gass_ep_cols_lds(int T, int K, int env_size, bool env_in_lds) {
  const size_t n = (size_t)T * K;
  return (4 * n + (size_t)T * (K * (K + 1) / 2) + (size_t)T * K + (env_in_lds ? (size_t)env_size : 0)) * sizeof(double) +
         2 * n * sizeof(int);
}

#ifdef BTF_GASS_EP_UNIT
__device__ __forceinline__ double gep_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// ------------------------------------------------------------------------------------------------------------- rows
template <int K>
__global__ __launch_bounds__(GEP_THREADS) void gass_ep_rows_kernel(GassEpArgs a) {
  constexpr int KK = K * (K + 1) / 2, NQ = KK + K + 1;
  __shared__ double part[GEP_THREADS / WAVE][NQ];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int d = i + 1 < K ? i + 1 : K;
  const int MT = a.M * a.T;
  double w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = k < d ? a.W[(size_t)i * K + k] : 0.0;
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  const double2* __restrict__ ep = a.ep + (size_t)i * MT;
  for (int e = tid; e < MT; e += GEP_THREADS) {
    const double2 mp = ep[e];
    const double* __restrict__ v = a.V + (size_t)e * K;
    double vv[K];
    double tau = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) { vv[k] = k < d ? v[k] : 0.0; tau = fma(w[k], vv[k], tau); }
    int q = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double pv = mp.y * vv[k];
#pragma unroll
      for (int l = 0; l <= k; ++l) { acc[q] = fma(pv, vv[l], acc[q]); ++q; }
    }
    const double pm = mp.y * mp.x;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[KK + k] = fma(pm, vv[k], acc[KK + k]);
    const double r = tau - mp.x;
    acc[NQ - 1] = fma(mp.y * r, r, acc[NQ - 1]);
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double s = gep_wave_sum(acc[q]);
    if (lane == 0) part[wave][q] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  // the tail in thread 0, its arrays in LDS (indexed by the row's d: no register arrays with dynamic indices)
  __shared__ double S[NQ], L[KK], y[K], mu[K], nu[K];
  for (int q = 0; q < NQ; ++q) {
    double s = 0.0;
    for (int u = 0; u < GEP_THREADS / WAVE; ++u) s += part[u][q];
    S[q] = s;
  }
  const double s2 = a.sigma2_dev ? *a.sigma2_dev : a.sigma2;
  // L L' = Q over the first d dimensions (packed lower triangle, row k at k(k+1)/2)
  bool ok = true;
  for (int k = 0; k < d; ++k) {
    for (int l = 0; l <= k; ++l) {
      double s = S[k * (k + 1) / 2 + l] + (l == k ? 1.0 / s2 : 0.0);
      for (int m = 0; m < l; ++m) s -= L[k * (k + 1) / 2 + m] * L[l * (l + 1) / 2 + m];
      if (l == k) { ok = ok && s > 0.0; L[k * (k + 1) / 2 + k] = sqrt(s > 0.0 ? s : 1.0); }
      else L[k * (k + 1) / 2 + l] = s / L[l * (l + 1) / 2 + l];
    }
  }
  if (!ok && atomicCAS(&a.status[0], 0, 1) == 0) a.status[1] = -21;
  // mean: L y = b, L' mu = y;  proposal: L' v = z
  const long long zo = w_z_offset(i, K);
  for (int k = 0; k < K; ++k) {
    nu[k] = k < d ? (a.z ? a.z[zo + k] : philox_normal(a.seed, a.stream, (unsigned long long)(zo + k))) : 0.0;
    mu[k] = 0.0;
  }
  for (int k = 0; k < d; ++k) {
    double s = S[KK + k];
    for (int l = 0; l < k; ++l) s -= L[k * (k + 1) / 2 + l] * y[l];
    y[k] = s / L[k * (k + 1) / 2 + k];
  }
  for (int k = d - 1; k >= 0; --k) {
    double s = y[k], t = nu[k];
    for (int l = k + 1; l < d; ++l) { s -= L[l * (l + 1) / 2 + k] * mu[l]; t -= L[l * (l + 1) / 2 + k] * nu[l]; }
    mu[k] = s / L[k * (k + 1) / 2 + k];
    nu[k] = t / L[k * (k + 1) / 2 + k];
  }
  for (int k = 0; k < K; ++k) {
    const size_t o = (size_t)i * K + k;
    a.X0[o] = a.W[o] - mu[k];
    a.Nu[o] = nu[k];
    a.Mu[o] = mu[k];
  }
  a.corr[i] = fma(0.5, S[NQ - 1], a.cconst[i]);
}

// ---------------------------------------------------------------------------------------------------------- columns
// The twisted elimination order (depth-major g = t K + k): depths 0..ts-1 ascending, T-1..ts+S descending, then the
// S = TF+1 separator depths; ts = (T - S) / 2.
__device__ __forceinline__ int gep_ord(int r, int n, int nl, int nsep) {
  return r < nl ? r : (r < nsep ? n - 1 - (r - nl) : nl + (r - nsep));
}
__device__ __forceinline__ int gep_pos(int g, int n, int nl, int nsep) {
  const int sk = n - nsep;
  return g < nl ? g : (g >= nl + sk ? nl + (n - 1 - g) : nsep + (g - nl));
}

// dynamic LDS: [env (env_size, unless in HBM)] [y1 n] [y2 n] [x1 n] [x2 n] [G T*KK] [h T*K] [ints: f n, off n]
template <int K>
__global__ __launch_bounds__(GEP_THREADS) void gass_ep_cols_kernel(GassEpArgs a) {
  constexpr int KK = K * (K + 1) / 2, NQ = KK + K;
  extern __shared__ double dyn[];
  __shared__ double qpart[GEP_THREADS / WAVE];
  const int j = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int T = a.T, N = a.N, n = T * K;
  double* env = a.env_g ? a.env_g + (size_t)j * a.env_size : dyn;
  double* y1 = (a.env_g ? dyn : dyn + a.env_size);
  double* y2 = y1 + n;
  double* x1 = y2 + n;
  double* x2 = x1 + n;
  double* G = x2 + n;
  double* h = G + (size_t)T * KK;
  int* ef = reinterpret_cast<int*>(h + (size_t)T * K);
  int* eo = ef + n;
  for (int r = tid; r < n; r += GEP_THREADS) { ef[r] = a.env_f[r]; eo[r] = a.env_off[r]; }
  for (int e = tid; e < a.env_size; e += GEP_THREADS) env[e] = 0.0;
  // per-depth blocks: a wave per depth, lanes over rows in order
  double qacc = 0.0;
  const double* __restrict__ Vj = a.V + (size_t)j * n;
  for (int t = wave; t < T; t += GEP_THREADS / WAVE) {
    double vt[K];
#pragma unroll
    for (int k = 0; k < K; ++k) vt[k] = Vj[(size_t)t * K + k];
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    const double2* __restrict__ ep = a.ep + ((size_t)j * T + t) * N;
    for (int i = lane; i < N; i += WAVE) {
      const double2 mp = ep[i];
      double w[K];
      double tau = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) { w[k] = a.W[(size_t)i * K + k]; tau = fma(w[k], vt[k], tau); }
      int q = 0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double pw = mp.y * w[k];
#pragma unroll
        for (int l = 0; l <= k; ++l) { acc[q] = fma(pw, w[l], acc[q]); ++q; }
      }
      const double pm = mp.y * mp.x;
#pragma unroll
      for (int k = 0; k < K; ++k) acc[KK + k] = fma(pm, w[k], acc[KK + k]);
      const double r = tau - mp.x;
      qacc = fma(mp.y * r, r, qacc);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const double s = gep_wave_sum(acc[q]);
      if (lane == 0) { if (q < KK) G[(size_t)t * KK + q] = s; else h[(size_t)t * K + q - KK] = s; }
    }
  }
  qacc = gep_wave_sum(qacc);
  if (lane == 0) qpart[wave] = qacc;
  __syncthreads();
  // P Q P' into the envelope, row by row (a thread owns a row: no races); the right-hand sides in elimination order
  const int S = a.TF + 1, ts = (T - S) / 2, nl = ts * K, nsep = n - S * K, D1 = a.TF + 2;
  const double* __restrict__ pb = a.pband + (size_t)j * T * D1;
  for (int r = tid; r < n; r += GEP_THREADS) {
    const int g = gep_ord(r, n, nl, nsep), t = g / K, k = g - t * K;
    double* row = env + eo[r] - ef[r];
    for (int l = 0; l < K; ++l) {
      const int c = gep_pos(t * K + l, n, nl, nsep);
      if (c <= r) row[c] += G[(size_t)t * KK + (k >= l ? k * (k + 1) / 2 + l : l * (l + 1) / 2 + k)];
    }
    for (int dd = 0; dd < D1; ++dd) {
      if (dd == 0) { row[r] += pb[(size_t)t * D1]; continue; }
      if (t + dd < T) { const int c = gep_pos((t + dd) * K + k, n, nl, nsep); if (c < r) row[c] += pb[(size_t)t * D1 + dd]; }
      if (t - dd >= 0) { const int c = gep_pos((t - dd) * K + k, n, nl, nsep); if (c < r) row[c] += pb[(size_t)(t - dd) * D1 + dd]; }
    }
    y1[r] = h[(size_t)t * K + k];
    y2[r] = a.z ? a.z[(size_t)j * n + r] : philox_normal(a.seed, a.stream, (unsigned long long)j * n + r);
  }
  // right-looking Cholesky inside the envelope: A(r,c) -= A(r,p) A(c,p) / A(p,p) for the candidates r >= c > p of
  // pivot p (the next bwe rows before the separator, then the separator rows), the column scaled afterwards
  auto ncand = [&](int p, int& na) {
    const int hiA = min(p + a.bwe, nsep - 1);
    na = hiA > p ? hiA - p : 0;
    const int s0 = max(p + 1, nsep);
    return na + (n - s0);
  };
  auto cand = [&](int p, int na, int q) { return q < na ? p + 1 + q : max(p + 1, nsep) + (q - na); };
  bool bad = false;
  for (int p = 0; p < n; ++p) {
    __syncthreads();
    const double piv = env[eo[p] + p - ef[p]];
    if (!(piv > 0.0)) { bad = true; continue; }
    const double ip = 1.0 / piv;
    int na;
    const int m = ncand(p, na);
    const int npair = m * (m + 1) / 2;
    for (int u = tid; u < npair; u += GEP_THREADS) {
      int q1 = (int)((sqrt(8.0 * u + 1.0) - 1.0) * 0.5);
      while (q1 * (q1 + 1) / 2 > u) --q1;
      while ((q1 + 1) * (q1 + 2) / 2 <= u) ++q1;
      const int q2 = u - q1 * (q1 + 1) / 2;
      const int r = cand(p, na, q1), c = cand(p, na, q2);
      if (ef[r] > p || ef[c] > p) continue;
      const double arp = env[eo[r] + p - ef[r]], acp = env[eo[c] + p - ef[c]];
      env[eo[r] + c - ef[r]] -= arp * acp * ip;
    }
  }
  __syncthreads();
  if (bad && tid == 0 && atomicCAS(&a.status[0], 0, 1) == 0) a.status[1] = -22;
  for (int r = tid; r < n; r += GEP_THREADS) {      // diagonal first: the scaling below reads it
    double* d = env + eo[r] + r - ef[r];
    *d = sqrt(*d > 0.0 ? *d : 1.0);
  }
  __syncthreads();
  for (int r = tid; r < n; r += GEP_THREADS)
    for (int c = ef[r]; c < r; ++c) env[eo[r] + c - ef[r]] /= env[eo[c] + c - ef[c]];
  // L y = b (column by column)
  for (int p = 0; p < n; ++p) {
    __syncthreads();
    const double yp = y1[p] / env[eo[p] + p - ef[p]];
    if (tid == 0) x1[p] = yp;
    int na;
    const int m = ncand(p, na);
    for (int q = tid; q < m; q += GEP_THREADS) {
      const int r = cand(p, na, q);
      if (ef[r] <= p) y1[r] -= env[eo[r] + p - ef[r]] * yp;
    }
  }
  __syncthreads();
  for (int r = tid; r < n; r += GEP_THREADS) y1[r] = x1[r];
  // L' mu = y and L' v = z (row by row from the last: the solved unknown leaves the rows' envelopes)
  for (int r = n - 1; r >= 0; --r) {
    __syncthreads();
    const double dg = env[eo[r] + r - ef[r]];
    const double m1 = y1[r] / dg, m2 = y2[r] / dg;
    if (tid == 0) { x1[r] = m1; x2[r] = m2; }
    for (int c = ef[r] + tid; c < r; c += GEP_THREADS) {
      const double l = env[eo[r] + c - ef[r]];
      y1[c] -= l * m1;
      y2[c] -= l * m2;
    }
  }
  __syncthreads();
  for (int r = tid; r < n; r += GEP_THREADS) {
    const size_t o = (size_t)j * n + gep_ord(r, n, nl, nsep);
    a.X0[o] = a.V[o] - x1[r];
    a.Nu[o] = x2[r];
    a.Mu[o] = x1[r];
  }
  if (tid == 0) {
    double s = 0.0;
    for (int u = 0; u < GEP_THREADS / WAVE; ++u) s += qpart[u];
    a.corr[j] = fma(0.5, s, a.cconst[j]);
  }
}

__global__ void gass_ep_fix_kernel(const double* __restrict__ corr, int nchains, double* __restrict__ cur, double* __restrict__ hh) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nchains) return;
  cur[c] += corr[c];
  hh[c] += corr[c];
}

__global__ void gass_ep_commit_kernel(const double* __restrict__ x0, const double* __restrict__ nu, const double* __restrict__ mu,
                                             double* __restrict__ x, long long n, int per, const double* __restrict__ theta,
                                             const int* __restrict__ keep) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e / per);
  if (keep[c]) return;
  double sn, cs;
  sincos(theta[c], &sn, &cs);
  x[e] = fma(x0[e], cs, nu[e] * sn) + mu[e];
}

#endif  // BTF_GASS_EP_UNIT

}  // namespace btf
