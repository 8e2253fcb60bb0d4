// Non-negative tensor factorisation and the factor PAV projection (btf_nmf.h): kernels and the btf_nmf_* entry points of
// include/btf.h, one compilation unit of their own.  gfx950 only.
#include "../../include/btf.h"
#include "btf_nmf.h"
#include "btf_scratch.h"      // Scratch: the device buffers of btf_nmf_pav

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>

namespace btf {
int set_global_error(int code, const std::string& msg);   // btf_abi.hip: the text btf_last_error(NULL) returns
}

using namespace btf;

struct btf_nmf {
  int dev = 0;
  hipStream_t stream = nullptr;
  int N = 0, M = 0, T = 0, R = 1, K = 0, MT = 0;
  bool miss = false;
  double ssw = 0.0;
  double* S = nullptr; unsigned char* C = nullptr;
  double* W = nullptr; double* V = nullptr;
  double* partW = nullptr; double* partV = nullptr; double* gpart = nullptr; double* rpart = nullptr;
  double* hist = nullptr; int hist_len = 0;
  NmfState* st = nullptr;
  int nchW = 0, VR = 0, nrcV = 0, nrss = 0;
};

namespace {

int fail(int code, const std::string& msg) { return set_global_error(code, msg); }

#define NMFCHK(call)                                                                                        \
  do {                                                                                                      \
    hipError_t e__ = (call);                                                                                \
    if (e__ != hipSuccess) return fail(BTF_EHIP, std::string(#call) + ": " + hipGetErrorString(e__));      \
  } while (0)

constexpr int wpart_rows(bool miss) { return miss ? 1 : 4; }

template <int K, bool MISS>
void launch_step(btf_nmf* h, const NmfArgs& a, int step, bool fit_W, bool fit_V, bool monotone) {
  constexpr int RB = wpart_rows(MISS);
  if (fit_W) {
    if (!MISS) hipLaunchKernelGGL(nmf_gram_kernel<K>, dim3(NMF_GP), dim3(256), 0, h->stream, (const double*)h->V, h->MT, h->gpart, (const NmfState*)h->st);
    hipLaunchKernelGGL((nmf_wpart_kernel<K, RB, MISS>), dim3((h->N + RB - 1) / RB, h->nchW), dim3(WAVE), 0, h->stream, a);
    hipLaunchKernelGGL((nmf_wsolve_kernel<K, MISS>), dim3((h->N + WAVE - 1) / WAVE), dim3(WAVE), 0, h->stream, a);
  }
  if (fit_V) {
    if (!MISS) hipLaunchKernelGGL(nmf_gram_kernel<K>, dim3(NMF_GP), dim3(256), 0, h->stream, (const double*)h->W, h->N, h->gpart, (const NmfState*)h->st);
    hipLaunchKernelGGL((nmf_vpart_kernel<K, MISS>), dim3((h->MT + WAVE - 1) / WAVE, h->nrcV), dim3(WAVE), 0, h->stream, a);
    hipLaunchKernelGGL((nmf_vsolve_kernel<K, MISS>), dim3((h->MT + WAVE - 1) / WAVE), dim3(WAVE), 0, h->stream, a);
    if (monotone)
      hipLaunchKernelGGL(nmf_pav_kernel<K>, dim3(h->M), dim3(256), (size_t)h->T * K * sizeof(double) + (size_t)h->T * sizeof(int),
                         h->stream, (const double*)h->W, h->V, h->N, h->T, (const NmfState*)h->st);
  }
  hipLaunchKernelGGL((nmf_rss_kernel<K, MISS>), dim3((h->MT + WAVE - 1) / WAVE, h->nrcV), dim3(WAVE), 0, h->stream, a);
  hipLaunchKernelGGL(nmf_decide_kernel, dim3(1), dim3(256), 0, h->stream, a, step);
}

template <int K>
void launch_step_k(btf_nmf* h, const NmfArgs& a, int step, bool fit_W, bool fit_V, bool monotone) {
  if (h->miss) launch_step<K, true>(h, a, step, fit_W, fit_V, monotone);
  else launch_step<K, false>(h, a, step, fit_W, fit_V, monotone);
}

void launch_step_any(btf_nmf* h, const NmfArgs& a, int step, bool fit_W, bool fit_V, bool monotone) {
  switch (h->K) {
    case 1: launch_step_k<1>(h, a, step, fit_W, fit_V, monotone); break;
    case 2: launch_step_k<2>(h, a, step, fit_W, fit_V, monotone); break;
    case 3: launch_step_k<3>(h, a, step, fit_W, fit_V, monotone); break;
    case 4: launch_step_k<4>(h, a, step, fit_W, fit_V, monotone); break;
    case 5: launch_step_k<5>(h, a, step, fit_W, fit_V, monotone); break;
    case 6: launch_step_k<6>(h, a, step, fit_W, fit_V, monotone); break;
    case 7: launch_step_k<7>(h, a, step, fit_W, fit_V, monotone); break;
    case 8: launch_step_k<8>(h, a, step, fit_W, fit_V, monotone); break;
    case 9: launch_step_k<9>(h, a, step, fit_W, fit_V, monotone); break;
    case 10: launch_step_k<10>(h, a, step, fit_W, fit_V, monotone); break;
    default: break;
  }
}

void launch_pav(int K, dim3 grid, size_t lds, hipStream_t s, const double* W, double* V, int N, int T) {
  switch (K) {
#define NMF_PAV_CASE(KT) case KT: hipLaunchKernelGGL(nmf_pav_kernel<KT>, grid, dim3(256), lds, s, W, V, N, T, (const NmfState*)nullptr); break;
    NMF_PAV_CASE(1) NMF_PAV_CASE(2) NMF_PAV_CASE(3) NMF_PAV_CASE(4) NMF_PAV_CASE(5)
    NMF_PAV_CASE(6) NMF_PAV_CASE(7) NMF_PAV_CASE(8) NMF_PAV_CASE(9) NMF_PAV_CASE(10)
#undef NMF_PAV_CASE
    default: break;
  }
}

// the PAV kernel holds one column in LDS
bool pav_fits(int T, int K) { return (size_t)T * K * sizeof(double) + (size_t)T * sizeof(int) <= 64 * 1024; }

}  // namespace

extern "C" {

int btf_nmf_create(btf_nmf** out, int device, int nrows, int ncols, int ndepth, int nreps, int nembeds, const double* S,
                   const unsigned char* counts, double ssw) {
  if (!out) return fail(BTF_EINVAL, "btf_nmf_create: out is NULL");
  *out = nullptr;
  if (nrows < 1 || ncols < 1 || ndepth < 1 || nreps < 1 || nreps > 255 || nembeds < 1 || nembeds > NMF_MAX_K || !S ||
      !(ssw >= 0.0) || (long long)ncols * ndepth > INT32_MAX / 2 || (long long)nrows * ncols * ndepth > (1LL << 40))
    return fail(BTF_EINVAL, "bad btf_nmf_create arguments");
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return fail(BTF_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  btf_nmf* h = new btf_nmf;
  h->dev = device;
  h->N = nrows; h->M = ncols; h->T = ndepth; h->R = nreps; h->K = nembeds; h->MT = ncols * ndepth;
  h->miss = counts != nullptr;
  h->ssw = ssw;
  const size_t cells = (size_t)h->N * h->MT;
  const int K = h->K, NA = K + (h->miss ? K * (K + 1) / 2 : 0);
  h->nchW = (h->MT + NMF_WCH - 1) / NMF_WCH;
  h->VR = h->N <= 1024 ? 64 : 256;          // rows per V-pass wave: enough waves at C3, a bounded partial slab at C5
  h->nrcV = (h->N + h->VR - 1) / h->VR;
  h->nrss = (h->MT + WAVE - 1) / WAVE * h->nrcV;
  auto bail = [&](hipError_t err, const char* what) {
    btf_nmf_destroy(h);
    return fail(BTF_EHIP, std::string(what) + ": " + hipGetErrorString(err));
  };
#define NMFA(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return bail(e__, #call); } while (0)
  NMFA(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  NMFA(hipMalloc((void**)&h->S, cells * sizeof(double)));
  if (h->miss) NMFA(hipMalloc((void**)&h->C, cells));
  NMFA(hipMalloc((void**)&h->W, (size_t)h->N * K * sizeof(double)));
  NMFA(hipMalloc((void**)&h->V, (size_t)h->MT * K * sizeof(double)));
  NMFA(hipMalloc((void**)&h->partW, (size_t)h->nchW * NA * h->N * sizeof(double)));
  NMFA(hipMalloc((void**)&h->partV, (size_t)h->nrcV * NA * h->MT * sizeof(double)));
  NMFA(hipMalloc((void**)&h->gpart, (size_t)NMF_GP * K * (K + 1) / 2 * sizeof(double)));
  NMFA(hipMalloc((void**)&h->rpart, (size_t)h->nrss * sizeof(double)));
  NMFA(hipMalloc((void**)&h->st, sizeof(NmfState)));
  NMFA(hipMemcpyAsync(h->S, S, cells * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (h->miss) NMFA(hipMemcpyAsync(h->C, counts, cells, hipMemcpyHostToDevice, h->stream));
  NMFA(hipStreamSynchronize(h->stream));
#undef NMFA
  *out = h;
  return BTF_OK;
}

void btf_nmf_destroy(btf_nmf* h) {
  if (!h) return;
  (void)hipSetDevice(h->dev);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : {(void*)h->S, (void*)h->C, (void*)h->W, (void*)h->V, (void*)h->partW, (void*)h->partV, (void*)h->gpart,
                  (void*)h->rpart, (void*)h->hist, (void*)h->st})
    if (p) (void)hipFree(p);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int btf_nmf_run(btf_nmf* h, double* W, double* V, int fit_W, int fit_V, int monotone, int max_steps, double tol, int verbose,
                int* steps_out, double* rmse_out, double* device_ms) {
  if (!h || !W || !V || !steps_out || max_steps < 0 || (max_steps > 0 && !rmse_out) || std::isnan(tol))
    return fail(BTF_EINVAL, "bad btf_nmf_run arguments");
  if (monotone && fit_V && !pav_fits(h->T, h->K)) return fail(BTF_EINVAL, "btf_nmf_run: ndepth * nembeds too large for the PAV kernel");
  NMFCHK(hipSetDevice(h->dev));
  const int K = h->K;
  if (max_steps > h->hist_len) {
    if (h->hist) NMFCHK(hipFree(h->hist));
    h->hist = nullptr;
    h->hist_len = 0;
    NMFCHK(hipMalloc((void**)&h->hist, (size_t)max_steps * sizeof(double)));
    h->hist_len = max_steps;
  }
  NmfState st0{0, 0, 0, -1, INFINITY, 0.0};
  NMFCHK(hipMemcpyAsync(h->W, W, (size_t)h->N * K * sizeof(double), hipMemcpyHostToDevice, h->stream));
  NMFCHK(hipMemcpyAsync(h->V, V, (size_t)h->MT * K * sizeof(double), hipMemcpyHostToDevice, h->stream));
  NMFCHK(hipMemcpyAsync(h->st, &st0, sizeof(NmfState), hipMemcpyHostToDevice, h->stream));
  NmfArgs a;
  a.S = h->S; a.C = h->C; a.W = h->W; a.V = h->V;
  a.partW = h->partW; a.partV = h->partV; a.gpart = h->gpart; a.rpart = h->rpart; a.hist = h->hist; a.st = h->st;
  a.N = h->N; a.MT = h->MT; a.R = h->R; a.nchW = h->nchW; a.VR = h->VR; a.nrcV = h->nrcV; a.nrss = h->nrss;
  a.ssw = h->ssw; a.tol = tol;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (device_ms) {
    NMFCHK(hipEventCreate(&e0));
    NMFCHK(hipEventCreate(&e1));
    NMFCHK(hipEventRecord(e0, h->stream));
  }
  NmfState st{};
  for (int step = 0; step < max_steps; ++step) {
    if (verbose) { printf("Step %d\n", step); fflush(stdout); }
    launch_step_any(h, a, step, fit_W != 0, fit_V != 0, monotone != 0);
    NMFCHK(hipGetLastError());
    if (verbose) {
      NMFCHK(hipMemcpyAsync(&st, h->st, sizeof(NmfState), hipMemcpyDeviceToHost, h->stream));
      NMFCHK(hipStreamSynchronize(h->stream));
      if (st.steps == step + 1) { printf("delta: %.17g\n", st.delta); fflush(stdout); }
      if (st.stop) break;
    }
  }
  if (device_ms) NMFCHK(hipEventRecord(e1, h->stream));
  NMFCHK(hipMemcpyAsync(&st, h->st, sizeof(NmfState), hipMemcpyDeviceToHost, h->stream));
  NMFCHK(hipMemcpyAsync(W, h->W, (size_t)h->N * K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  NMFCHK(hipMemcpyAsync(V, h->V, (size_t)h->MT * K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (max_steps > 0) NMFCHK(hipMemcpyAsync(rmse_out, h->hist, (size_t)max_steps * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  NMFCHK(hipStreamSynchronize(h->stream));
  if (device_ms) {
    float ms = 0.f;
    NMFCHK(hipEventElapsedTime(&ms, e0, e1));
    *device_ms = ms;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  *steps_out = st.steps;
  if (st.err) {
    const bool inW = st.err_index < h->N;
    const int idx = inW ? st.err_index : st.err_index - h->N;
    char buf[160];
    snprintf(buf, sizeof buf, "tensor_nmf: the NNLS of %s %d %s", inW ? "row" : "cell (j*T + t)", idx,
             (st.err & NMF_ERR_ITER) ? "reached the iteration cap (3 x unknowns)" : "gave a non-finite solution");
    return fail(BTF_EINVAL, buf);
  }
  return BTF_OK;
}

int btf_nmf_pav(int device, int nrows, int ncols, int ndepth, int nembeds, const double* W, double* V) {
  if (nrows < 1 || ncols < 1 || ndepth < 1 || nembeds < 1 || nembeds > NMF_MAX_K || !W || !V)
    return fail(BTF_EINVAL, "bad btf_nmf_pav arguments");
  if (!pav_fits(ndepth, nembeds)) return fail(BTF_EINVAL, "btf_nmf_pav: ndepth * nembeds too large for the PAV kernel");
  NMFCHK(hipSetDevice(device));
  const size_t nW = (size_t)nrows * nembeds, nV = (size_t)ncols * ndepth * nembeds;
  Scratch s(nullptr, nullptr);
  const double* dW = s.upload(W, nW);
  double* dV = s.upload(V, nV);
  if (s.rc()) return s.rc();
  launch_pav(nembeds, dim3(ncols), (size_t)ndepth * nembeds * sizeof(double) + (size_t)ndepth * sizeof(int), 0, dW, dV, nrows, ndepth);
  s.check(hipGetLastError(), "hipGetLastError (nmf_pav_kernel)");
  s.download(V, dV, nV);
  return s.finish();
}

}  // extern "C"
