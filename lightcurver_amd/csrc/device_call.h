// Ownership of device buffers on the host side of liblcmi: a pool that frees what it allocated, the per-call object the
// stamp-level entry points are written with, and the growth of a device-resident history buffer.  Every method returns
// hipError_t, so call sites read LC_HIP(ctx, ...), and an early return frees everything.
#pragma once
#include <algorithm>
#include <vector>

#include "lc_common.h"

namespace lc {

// device buffers that live as long as the pool: one call, or one batch object
struct DevPool {
  std::vector<void *> held;
  DevPool() = default;
  DevPool(const DevPool &) = delete;
  DevPool &operator=(const DevPool &) = delete;
  ~DevPool() {
    for (void *p : held) (void)hipFree(p);
  }
  template <class T>
  hipError_t alloc(size_t count, T **d) {
    hipError_t e = hipMalloc((void **)d, count * sizeof(T));
    if (e == hipSuccess) held.push_back(*d);
    return e;
  }
  template <class T>
  hipError_t alloc_zeroed(size_t count, T **d, hipStream_t stream) {
    hipError_t e = alloc(count, d);
    return e == hipSuccess ? hipMemsetAsync(*d, 0, count * sizeof(T), stream) : e;
  }
  // frees one buffer ahead of the pool (a null pointer, or one the pool does not hold, is left alone)
  void release(void *p) {
    const auto it = std::find(held.begin(), held.end(), p);
    if (!p || it == held.end()) return;
    held.erase(it);
    (void)hipFree(p);
  }
};

// One call of an entry point on ctx->stream: inputs up, ev0, kernels, ev1, outputs back, one synchronise.
//   DeviceCall call(ctx);
//   LC_HIP(ctx, call.upload(host_in, count, &d_in));     // a null host pointer gives a null device pointer
//   LC_HIP(ctx, call.result(host_out, count, &d_out));   // likewise: an output the caller did not ask for
//   LC_HIP(ctx, call.alloc(count, &d_scratch));          // neither input nor output
//   call.download(host_out, count, d_resident);          // an output that lies in a buffer the call does not own
//   LC_HIP(ctx, call.start());  ... launches ...  LC_HIP(ctx, call.stop());
//   LC_HIP(ctx, call.finish(kernel_ms));
class DeviceCall {
 public:
  explicit DeviceCall(lc_ctx *ctx) : ctx_(ctx) {}
  template <class T>
  hipError_t alloc(size_t count, T **d) {
    return pool_.alloc(count, d);
  }
  template <class T>
  hipError_t upload(const T *host, size_t count, const T **d) {
    T *p = nullptr;
    *d = nullptr;
    if (!host) return hipSuccess;
    hipError_t e = pool_.alloc(count, &p);
    if (e != hipSuccess) return e;
    *d = p;
    return hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, ctx_->stream);
  }
  template <class T>
  hipError_t result(T *host, size_t count, T **d) {
    *d = nullptr;
    if (!host) return hipSuccess;
    hipError_t e = pool_.alloc(count, d);
    if (e == hipSuccess) back_.push_back({host, *d, count * sizeof(T)});
    return e;
  }
  template <class T>
  void download(T *host, size_t count, const T *d) {
    if (host) back_.push_back({host, d, count * sizeof(T)});
  }
  hipError_t start() { return hipEventRecord(ctx_->ev0, ctx_->stream); }
  hipError_t stop() { return hipEventRecord(ctx_->ev1, ctx_->stream); }
  // the registered outputs in the order of their registration, the synchronise, then the time between start and stop
  hipError_t finish(float *kernel_ms) {
    for (const Back &b : back_) {
      hipError_t e = hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, ctx_->stream);
      if (e != hipSuccess) return e;
    }
    hipError_t e = hipStreamSynchronize(ctx_->stream);
    if (e != hipSuccess || !kernel_ms) return e;
    return hipEventElapsedTime(kernel_ms, ctx_->ev0, ctx_->ev1);
  }

 private:
  struct Back {
    void *host;
    const void *dev;
    size_t bytes;
  };
  lc_ctx *ctx_;
  DevPool pool_;
  std::vector<Back> back_;
};

// Grows the device history *hist [rows][*stride] to hold `needed` columns: a zeroed buffer of max(needed, 2 * *stride +
// 64) columns takes the old columns of every row, the old buffer is freed and the new pointer and stride are published.
// On failure the new buffer is freed and *hist and *stride stay as they were.
inline hipError_t grow_history(float **hist, int *stride, int rows, int needed, hipStream_t stream) {
  if (needed <= *stride) return hipSuccess;
  const size_t os = (size_t)*stride * sizeof(float), ns = (size_t)std::max(needed, 2 * *stride + 64) * sizeof(float);
  float *nh = nullptr;
  hipError_t e = hipMalloc((void **)&nh, (size_t)rows * ns);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(nh, 0, (size_t)rows * ns, stream);
  if (e == hipSuccess && *hist) {
    e = rows == 1 ? hipMemcpyAsync(nh, *hist, os, hipMemcpyDeviceToDevice, stream)
                  : hipMemcpy2DAsync(nh, ns, *hist, os, os, rows, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
  }
  if (e != hipSuccess) {
    (void)hipFree(nh);
    return e;
  }
  if (*hist) (void)hipFree(*hist);
  *hist = nh;
  *stride = (int)(ns / sizeof(float));
  return hipSuccess;
}

}  // namespace lc
