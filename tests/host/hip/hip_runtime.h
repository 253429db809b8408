// A stand-in for <hip/hip_runtime.h> over malloc and memcpy, for host tests of csrc/device_call.h: the handful of types
// and calls that header and lc_common.h use, a counter that fails the k-th runtime call, and a count of live allocations.
// "Device" memory is host memory here, so a test reads and writes it directly.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>

#define __host__
#define __device__

typedef struct fake_stream *hipStream_t;
typedef struct fake_event *hipEvent_t;
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };

namespace fake_hip {
inline int calls = 0;    // runtime calls since reset() (hipFree and hipGetErrorString are not counted: they cannot fail)
inline int fail_at = 0;  // the call with this number fails (1-based; 0: none)
inline int live = 0;     // allocations not yet freed
inline int mallocs = 0;  // successful allocations since reset()
inline void reset(int fail) {
  calls = 0;
  mallocs = 0;
  fail_at = fail;
}
inline bool fails() { return ++calls == fail_at; }
}  // namespace fake_hip

inline const char *hipGetErrorString(hipError_t e) {
  return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "unknown error";
}
inline hipError_t hipSetDevice(int) { return fake_hip::fails() ? hipErrorUnknown : hipSuccess; }
inline hipError_t hipMalloc(void **p, size_t bytes) {
  if (fake_hip::fails()) return hipErrorOutOfMemory;
  *p = std::malloc(bytes ? bytes : 1);
  ++fake_hip::live;
  ++fake_hip::mallocs;
  return hipSuccess;
}
inline hipError_t hipFree(void *p) {
  if (p) --fake_hip::live;
  std::free(p);
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) {
  if (fake_hip::fails()) return hipErrorUnknown;
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}
inline hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                                   hipMemcpyKind, hipStream_t) {
  if (fake_hip::fails()) return hipErrorUnknown;
  for (size_t r = 0; r < height; ++r) std::memcpy((char *)dst + r * dpitch, (const char *)src + r * spitch, width);
  return hipSuccess;
}
inline hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t) {
  if (fake_hip::fails()) return hipErrorUnknown;
  std::memset(dst, value, bytes);
  return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return fake_hip::fails() ? hipErrorUnknown : hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return fake_hip::fails() ? hipErrorUnknown : hipSuccess; }
inline hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) {
  if (fake_hip::fails()) return hipErrorUnknown;
  *ms = 0.25f;
  return hipSuccess;
}
