// The device scratch of one entry-point call (host code only): every buffer the call allocates, freed on every path out.
#pragma once
#include "../../include/btf.h"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

namespace btf {

int report_error(btf_ctx* c, int code, const std::string& msg);   // btf_abi.hip: the text btf_last_error(c) returns; c may be null

// One hipMalloc per buffer, copies and launches on one stream (the stateless entry points: the null stream).  The first
// HIP call that fails is recorded as BTF_EHIP; from then on nothing is allocated, copied or launched - a kernel never
// sees the null pointer a failed allocation handed out - and rc() / finish() return that error.
class Scratch {
 public:
  Scratch(btf_ctx* c, hipStream_t st) : c_(c), st_(st) {}
  ~Scratch() { for (void* p : bufs_) (void)hipFree(p); }
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;

  btf_ctx* ctx() const { return c_; }
  hipStream_t stream() const { return st_; }
  int rc() const { return rc_; }

  // the result of a HIP call made on the scratch's behalf; false once anything has failed
  bool check(hipError_t e, const char* call) {
    if (e != hipSuccess && !rc_) rc_ = report_error(c_, BTF_EHIP, std::string(call) + ": " + hipGetErrorString(e));
    return !rc_;
  }
  template <typename T>
  T* alloc(size_t n) {
    void* p = nullptr;
    if (rc_ || !check(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)), "hipMalloc")) return nullptr;
    bufs_.push_back(p);
    return static_cast<T*>(p);
  }
  // the host array must stay alive until finish()
  template <typename T>
  T* upload(const T* h, size_t n) {
    T* d = alloc<T>(n);
    if (d) check(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, st_), "hipMemcpyAsync (upload)");
    return d;
  }
  template <typename T>
  void download(T* h, const T* d, size_t n) {
    if (h && !rc_) check(hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, st_), "hipMemcpyAsync (download)");
  }
  // zeroes `bytes` of one of its buffers on the stream
  void zero(void* p, size_t bytes) {
    if (!rc_) check(hipMemsetAsync(p, 0, bytes, st_), "hipMemsetAsync");
  }
  // a launch the profile does not count (launch_counted of btf_ctx.h: the counted one)
  template <typename F, typename... Args>
  void launch(F kernel, dim3 grid, dim3 block, size_t lds, Args... args) {
    if (rc_) return;
    hipLaunchKernelGGL(kernel, grid, block, (unsigned)lds, st_, args...);
    check(hipGetLastError(), "hipGetLastError (kernel launch)");
  }
  // the downloads are complete in host memory when this returns BTF_OK
  int finish() {
    if (!rc_) check(hipStreamSynchronize(st_), "hipStreamSynchronize");
    return rc_;
  }

 private:
  btf_ctx* c_;
  hipStream_t st_;
  int rc_ = BTF_OK;
  std::vector<void*> bufs_;
};

}  // namespace btf
