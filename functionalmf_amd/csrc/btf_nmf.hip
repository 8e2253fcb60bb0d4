// Non-negative tensor factorisation and the factor PAV projection (btf_nmf.h): kernels and the btf_nmf_* entry points of
// include/btf.h, one compilation unit of their own.  gfx950 only.
#include "../../include/btf.h"
#include "btf_nmf.h"
#include "btf_ctx.h"          // use_device; Scratch: the device buffers of btf_nmf_pav

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

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
  // bounds and row features (btf_nmf_set_bounds / btf_nmf_set_row_features)
  double max_entry = 0.0;                       // 0: no bound
  int F = 0;
  bool fmiss = false;
  double* SX = nullptr; unsigned char* CX = nullptr; unsigned char* fskip = nullptr;
  double* Rf = nullptr; double* partR = nullptr;
  unsigned char* flag = nullptr;                // [N + MT + F]: the systems projected in the last step run
  int* nproj = nullptr;                         // [hist_len]: projected systems per step
};

namespace {

int fail(int code, const std::string& msg) { return report_error(nullptr, code, msg); }   // the text btf_last_error(NULL) returns

#define NMFCHK(call)                                                                                        \
  do {                                                                                                      \
    hipError_t e__ = (call);                                                                                \
    if (e__ != hipSuccess) return fail(BTF_EHIP, std::string(#call) + ": " + hipGetErrorString(e__));      \
  } while (0)

constexpr int wpart_rows(bool miss) { return miss ? 1 : 4; }

// the arguments of one nmf_project_kernel launch
NmfProj proj_args(btf_nmf* h, double* X, const double* Cq, const double* part, int nsys, int nq, int nslab, bool rows, int base,
                  int step) {
  NmfProj p;
  p.X = X; p.Cq = Cq; p.part = part; p.flag = h->flag + base; p.nproj = h->nproj + step;
  p.nsys = nsys; p.nq = nq; p.nslab = nslab; p.rows = rows ? 1 : 0; p.err_base = base; p.hi = h->max_entry;
  return p;
}

template <int K, bool FM>
void launch_features(btf_nmf* h, const NmfArgs& af, int step) {
  if (!FM) hipLaunchKernelGGL(nmf_gram_kernel<K>, dim3(NMF_GP), dim3(256), 0, h->stream, (const double*)h->W, h->N, h->gpart, (const NmfState*)h->st);
  hipLaunchKernelGGL((nmf_vpart_kernel<K, FM>), dim3((h->F + WAVE - 1) / WAVE, h->nrcV), dim3(WAVE), 0, h->stream, af);
  hipLaunchKernelGGL((nmf_vsolve_kernel<K, FM>), dim3((h->F + WAVE - 1) / WAVE), dim3(WAVE), 0, h->stream, af);
  if (h->max_entry > 0.0)
    hipLaunchKernelGGL((nmf_project_kernel<K, FM>), dim3(h->F), dim3(WAVE), 0, h->stream, af,
                       proj_args(h, h->Rf, h->W, h->partR, h->F, h->N, h->nrcV, false, h->N + h->MT, step));
}

template <int K, bool MISS>
void launch_step(btf_nmf* h, const NmfArgs& a, const NmfArgs& af, int step, bool fit_W, bool fit_V, bool monotone) {
  constexpr int RB = wpart_rows(MISS);
  const bool bound = h->max_entry > 0.0;
  if (fit_W) {
    if (!MISS) hipLaunchKernelGGL(nmf_gram_kernel<K>, dim3(NMF_GP), dim3(256), 0, h->stream, (const double*)h->V, h->MT, h->gpart, (const NmfState*)h->st);
    hipLaunchKernelGGL((nmf_wpart_kernel<K, RB, MISS>), dim3((h->N + RB - 1) / RB, h->nchW), dim3(WAVE), 0, h->stream, a);
    hipLaunchKernelGGL((nmf_wsolve_kernel<K, MISS>), dim3((h->N + WAVE - 1) / WAVE), dim3(WAVE), 0, h->stream, a);
    if (bound)
      hipLaunchKernelGGL((nmf_project_kernel<K, MISS>), dim3(h->N), dim3(WAVE), 0, h->stream, a,
                         proj_args(h, h->W, h->V, h->partW, h->N, h->MT, h->nchW, true, 0, step));
  }
  if (fit_V) {
    if (!MISS) hipLaunchKernelGGL(nmf_gram_kernel<K>, dim3(NMF_GP), dim3(256), 0, h->stream, (const double*)h->W, h->N, h->gpart, (const NmfState*)h->st);
    hipLaunchKernelGGL((nmf_vpart_kernel<K, MISS>), dim3((h->MT + WAVE - 1) / WAVE, h->nrcV), dim3(WAVE), 0, h->stream, a);
    hipLaunchKernelGGL((nmf_vsolve_kernel<K, MISS>), dim3((h->MT + WAVE - 1) / WAVE), dim3(WAVE), 0, h->stream, a);
    if (bound)
      hipLaunchKernelGGL((nmf_project_kernel<K, MISS>), dim3(h->MT), dim3(WAVE), 0, h->stream, a,
                         proj_args(h, h->V, h->W, h->partV, h->MT, h->N, h->nrcV, false, h->N, step));
    if (monotone)
      hipLaunchKernelGGL(nmf_pav_kernel<K>, dim3(h->M), dim3(256), (size_t)h->T * K * sizeof(double) + (size_t)h->T * sizeof(int),
                         h->stream, (const double*)h->W, h->V, h->N, h->T, (const NmfState*)h->st);
  }
  if (h->F > 0) {
    if (h->fmiss) launch_features<K, true>(h, af, step);
    else launch_features<K, false>(h, af, step);
  }
  hipLaunchKernelGGL((nmf_rss_kernel<K, MISS>), dim3((h->MT + WAVE - 1) / WAVE, h->nrcV), dim3(WAVE), 0, h->stream, a);
  hipLaunchKernelGGL(nmf_decide_kernel, dim3(1), dim3(256), 0, h->stream, a, step);
}

template <int K>
void launch_step_k(btf_nmf* h, const NmfArgs& a, const NmfArgs& af, int step, bool fit_W, bool fit_V, bool monotone) {
  if (h->miss) launch_step<K, true>(h, a, af, step, fit_W, fit_V, monotone);
  else launch_step<K, false>(h, a, af, step, fit_W, fit_V, monotone);
}

void launch_step_any(btf_nmf* h, const NmfArgs& a, const NmfArgs& af, int step, bool fit_W, bool fit_V, bool monotone) {
  switch (h->K) {
    case 1: launch_step_k<1>(h, a, af, step, fit_W, fit_V, monotone); break;
    case 2: launch_step_k<2>(h, a, af, step, fit_W, fit_V, monotone); break;
    case 3: launch_step_k<3>(h, a, af, step, fit_W, fit_V, monotone); break;
    case 4: launch_step_k<4>(h, a, af, step, fit_W, fit_V, monotone); break;
    case 5: launch_step_k<5>(h, a, af, step, fit_W, fit_V, monotone); break;
    case 6: launch_step_k<6>(h, a, af, step, fit_W, fit_V, monotone); break;
    case 7: launch_step_k<7>(h, a, af, step, fit_W, fit_V, monotone); break;
    case 8: launch_step_k<8>(h, a, af, step, fit_W, fit_V, monotone); break;
    case 9: launch_step_k<9>(h, a, af, step, fit_W, fit_V, monotone); break;
    case 10: launch_step_k<10>(h, a, af, step, fit_W, fit_V, monotone); break;
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

// the ALS run behind btf_nmf_run and btf_nmf_run_bounded (include/btf.h)
int nmf_run(btf_nmf* h, double* W, double* V, double* Rf, int fit_W, int fit_V, int monotone, int max_steps, double tol,
            int verbose, int* steps_out, double* rmse_out, double* device_ms, unsigned char* flags_out, int* nproj_out) {
  if (!h || !W || !V || !steps_out || max_steps < 0 || (max_steps > 0 && !rmse_out) || std::isnan(tol))
    return fail(BTF_EINVAL, "bad btf_nmf_run arguments");
  if ((h->F > 0) != (Rf != nullptr))
    return fail(BTF_EINVAL, h->F > 0 ? "btf_nmf_run: row features are set: call btf_nmf_run_bounded with R"
                                     : "btf_nmf_run_bounded: R given without row features");
  if (monotone && fit_V && !pav_fits(h->T, h->K)) return fail(BTF_EINVAL, "btf_nmf_run: ndepth * nembeds too large for the PAV kernel");
  NMFCHK(hipSetDevice(h->dev));
  const int K = h->K;
  if (max_steps > h->hist_len) {
    if (h->hist) NMFCHK(hipFree(h->hist));
    if (h->nproj) NMFCHK(hipFree(h->nproj));
    h->hist = nullptr;
    h->nproj = nullptr;
    h->hist_len = 0;
    NMFCHK(hipMalloc((void**)&h->hist, (size_t)max_steps * sizeof(double)));
    NMFCHK(hipMalloc((void**)&h->nproj, (size_t)max_steps * sizeof(int)));
    h->hist_len = max_steps;
  }
  const size_t nflag = (size_t)h->N + h->MT + h->F;
  NMFCHK(hipMemsetAsync(h->flag, 0, nflag, h->stream));
  if (max_steps > 0) NMFCHK(hipMemsetAsync(h->nproj, 0, (size_t)max_steps * sizeof(int), h->stream));
  if (Rf) NMFCHK(hipMemcpyAsync(h->Rf, Rf, (size_t)h->F * K * sizeof(double), hipMemcpyHostToDevice, h->stream));
  NmfState st0{0, 0, 0, -1, INFINITY, 0.0};
  NMFCHK(hipMemcpyAsync(h->W, W, (size_t)h->N * K * sizeof(double), hipMemcpyHostToDevice, h->stream));
  NMFCHK(hipMemcpyAsync(h->V, V, (size_t)h->MT * K * sizeof(double), hipMemcpyHostToDevice, h->stream));
  NMFCHK(hipMemcpyAsync(h->st, &st0, sizeof(NmfState), hipMemcpyHostToDevice, h->stream));
  NmfArgs a{};
  a.S = h->S; a.C = h->C; a.W = h->W; a.V = h->V;
  a.partW = h->partW; a.partV = h->partV; a.gpart = h->gpart; a.rpart = h->rpart; a.hist = h->hist; a.st = h->st;
  a.N = h->N; a.MT = h->MT; a.R = h->R; a.nchW = h->nchW; a.VR = h->VR; a.nrcV = h->nrcV; a.nrss = h->nrss;
  a.ssw = h->ssw; a.tol = tol;
  a.Rf = h->Rf; a.SX = h->SX; a.CX = h->CX; a.F = h->F; a.skip = nullptr; a.err_base = h->N;
  NmfArgs af = a;                              // the fit of R: X is one more column of F cells with one replicate
  af.S = h->SX; af.C = h->CX; af.V = h->Rf; af.partV = h->partR; af.MT = h->F; af.R = 1; af.F = 0; af.skip = h->fskip;
  af.err_base = h->N + h->MT;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (device_ms) {
    NMFCHK(hipEventCreate(&e0));
    NMFCHK(hipEventCreate(&e1));
    NMFCHK(hipEventRecord(e0, h->stream));
  }
  NmfState st{};
  for (int step = 0; step < max_steps; ++step) {
    if (verbose) { printf("Step %d\n", step); fflush(stdout); }
    launch_step_any(h, a, af, step, fit_W != 0, fit_V != 0, monotone != 0);
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
  if (Rf) NMFCHK(hipMemcpyAsync(Rf, h->Rf, (size_t)h->F * K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (flags_out) NMFCHK(hipMemcpyAsync(flags_out, h->flag, nflag, hipMemcpyDeviceToHost, h->stream));
  if (nproj_out && max_steps > 0)
    NMFCHK(hipMemcpyAsync(nproj_out, h->nproj, (size_t)max_steps * sizeof(int), hipMemcpyDeviceToHost, h->stream));
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
    const int kind = st.err_index < h->N ? 0 : st.err_index < h->N + h->MT ? 1 : 2;
    const int idx = st.err_index - (kind == 0 ? 0 : kind == 1 ? h->N : h->N + h->MT);
    const char* what = (st.err & NMF_ERR_ITER)            ? "NNLS of %s %d reached the iteration cap (3 x unknowns)"
                       : (st.err & NMF_ERR_NONFINITE)     ? "NNLS of %s %d gave a non-finite solution"
                       : (st.err & NMF_ERR_QP_ITER)       ? "max_entry projection of %s %d reached the iteration cap (50 x (nembeds + 1))"
                       : (st.err & NMF_ERR_QP_INFEASIBLE) ? "max_entry projection of %s %d has no feasible point"
                                                          : "max_entry projection of %s %d has a singular A'A";
    char fmt[160], buf[224];
    snprintf(fmt, sizeof fmt, "tensor_nmf: the %s", what);
    snprintf(buf, sizeof buf, fmt, kind == 0 ? "row" : kind == 1 ? "cell (j*T + t)" : "row feature", idx);
    return fail(BTF_EINVAL, buf);
  }
  return BTF_OK;
}

}  // namespace

extern "C" {

int btf_nmf_create(btf_nmf** out, int device, int nrows, int ncols, int ndepth, int nreps, int nembeds, const double* S,
                   const unsigned char* counts, double ssw) {
  if (!out) return fail(BTF_EINVAL, "btf_nmf_create: out is NULL");
  *out = nullptr;
  if (nrows < 1 || ncols < 1 || ndepth < 1 || nreps < 1 || nreps > 255 || nembeds < 1 || nembeds > NMF_MAX_K || !S ||
      !(ssw >= 0.0) || (long long)ncols * ndepth > INT32_MAX / 2 || (long long)nrows * ncols * ndepth > (1LL << 40))
    return fail(BTF_EINVAL, "bad btf_nmf_create arguments");
  if (int rc = use_device(device)) return rc;
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
  NMFA(hipMalloc((void**)&h->flag, (size_t)h->N + h->MT));
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
                  (void*)h->rpart, (void*)h->hist, (void*)h->st, (void*)h->SX, (void*)h->CX, (void*)h->fskip, (void*)h->Rf,
                  (void*)h->partR, (void*)h->flag, (void*)h->nproj})
    if (p) (void)hipFree(p);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int btf_nmf_run(btf_nmf* h, double* W, double* V, int fit_W, int fit_V, int monotone, int max_steps, double tol, int verbose,
                int* steps_out, double* rmse_out, double* device_ms) {
  return nmf_run(h, W, V, nullptr, fit_W, fit_V, monotone, max_steps, tol, verbose, steps_out, rmse_out, device_ms, nullptr, nullptr);
}

int btf_nmf_run_bounded(btf_nmf* h, double* W, double* V, double* R, int fit_W, int fit_V, int monotone, int max_steps,
                        double tol, int verbose, int* steps_out, double* rmse_out, double* device_ms,
                        unsigned char* projected_out, int* nprojected_out) {
  return nmf_run(h, W, V, R, fit_W, fit_V, monotone, max_steps, tol, verbose, steps_out, rmse_out, device_ms, projected_out,
                 nprojected_out);
}

int btf_nmf_set_bounds(btf_nmf* h, double max_entry) {
  if (!h || !(max_entry >= 0.0) || std::isinf(max_entry)) return fail(BTF_EINVAL, "btf_nmf_set_bounds: max_entry must be positive and finite, or 0 for none");
  h->max_entry = max_entry;
  return BTF_OK;
}

int btf_nmf_set_row_features(btf_nmf* h, int nfeatures, const double* X, const unsigned char* observed) {
  if (!h || nfeatures < 0 || (nfeatures > 0 && !X)) return fail(BTF_EINVAL, "bad btf_nmf_set_row_features arguments");
  NMFCHK(hipSetDevice(h->dev));
  NMFCHK(hipStreamSynchronize(h->stream));
  for (void** p : {(void**)&h->SX, (void**)&h->CX, (void**)&h->fskip, (void**)&h->Rf, (void**)&h->partR, (void**)&h->flag}) {
    if (*p) NMFCHK(hipFree(*p));
    *p = nullptr;
  }
  h->F = 0;
  h->fmiss = false;
  const int F = nfeatures, K = h->K;
  NMFCHK(hipMalloc((void**)&h->flag, (size_t)h->N + h->MT + F));
  if (F == 0) return BTF_OK;
  const size_t nx = (size_t)h->N * F;
  const int NA = K + (observed ? K * (K + 1) / 2 : 0);
  std::vector<unsigned char> skip(F, 0);
  if (observed)
    for (int f = 0; f < F; ++f) {
      bool any = false;
      for (int i = 0; i < h->N && !any; ++i) any = observed[(size_t)i * F + f] != 0;
      skip[f] = any ? 0 : 1;
    }
  NMFCHK(hipMalloc((void**)&h->SX, nx * sizeof(double)));
  if (observed) NMFCHK(hipMalloc((void**)&h->CX, nx));
  NMFCHK(hipMalloc((void**)&h->fskip, (size_t)F));
  NMFCHK(hipMalloc((void**)&h->Rf, (size_t)F * K * sizeof(double)));
  NMFCHK(hipMalloc((void**)&h->partR, (size_t)h->nrcV * NA * F * sizeof(double)));
  NMFCHK(hipMemcpyAsync(h->SX, X, nx * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (observed) NMFCHK(hipMemcpyAsync(h->CX, observed, nx, hipMemcpyHostToDevice, h->stream));
  NMFCHK(hipMemcpyAsync(h->fskip, skip.data(), (size_t)F, hipMemcpyHostToDevice, h->stream));
  NMFCHK(hipStreamSynchronize(h->stream));
  h->F = F;
  h->fmiss = observed != nullptr;
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
