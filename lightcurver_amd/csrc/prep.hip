// Stamp pre-processing in one pass over the stack and a copy-bandwidth probe.
//
// One workgroup per stamp.  Per pixel it restates what the reference does on the host before the fits:
//   cutout_making.py:43-51             noisemap = max(sqrt((t rms)^2 + |t data|), 1e-7) / t      (t = exposure time)
//   roi_file_preparation.py:162-164    data, noisemap /= coefficient
//   psf_modelling.py:139-143           both NaN -> data 0, noisemap 1, pixel masked
//   roi_file_preparation.py:194-201    both NaN -> data 0, noisemap 1e7; noisemap[flagged] *= 1000
//   star_photometry.py:309-316         same, but a flagged pixel boosts the WHOLE epoch, once
//   psf_modelling.py:144-153           number of masked pixels per stamp (the caller applies the 40 % cut)
// and emits what the fit objects take: cleaned data, noise map, and weight = good / sigma^2.
#include <cmath>
#include <cstring>
#include <vector>

#include "device_call.h"
#include "lc_common.h"
#include "noise_pixel.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kPrepThreads = 256;

struct PrepArgs {
  int K, npix;
  const float *data, *noisemap, *rms, *exptime, *coefficient;
  const uint8_t *bad;
  float nan_noise, boost;
  int boost_whole_stamp;
  float *data_out, *noisemap_out, *weight_out;
  int32_t *masked_count;
};

__device__ __forceinline__ void prep_pixel(const PrepArgs &A, int k, size_t idx, float inv_coef, float t, float trms2,
                                           float &d, float &s, bool &flagged, bool &both_nan) {
  d = A.data[idx];
  if (A.noisemap) {
    s = A.noisemap[idx];
  } else {
    s = noise_from_rms(d, t, trms2);
  }
  d /= inv_coef;
  s /= inv_coef;
  both_nan = (d != d) && (s != s);
  if (both_nan) {
    d = 0.f;
    s = A.nan_noise;
  }
  flagged = A.bad ? (A.bad[idx] != 0) : false;
}

__global__ __launch_bounds__(kPrepThreads) void prep_stamps_kernel(PrepArgs A) {
  __shared__ int cnt[kPrepThreads / 64], flg[kPrepThreads / 64];
  __shared__ int tot[2];
  const int k = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)k * A.npix;
  const float inv_coef = A.coefficient ? A.coefficient[k] : 1.0f;  // the divisor itself: divisions are kept, as in the reference
  const float t = A.exptime ? A.exptime[k] : 1.0f;
  const float trms2 = A.rms ? noise_trms2(t, A.rms[k]) : 0.f;
  // pass 1: masked pixels of the stamp (flagged or NaN in both inputs), and whether anything is flagged
  int masked = 0, any = 0;
  for (int p = tid; p < A.npix; p += kPrepThreads) {
    float d, s;
    bool flagged, both_nan;
    prep_pixel(A, k, base + p, inv_coef, t, trms2, d, s, flagged, both_nan);
    masked += (flagged || both_nan) ? 1 : 0;
    any |= flagged ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    masked += __shfl_down(masked, off, 64);
    any |= __shfl_down(any, off, 64);
  }
  if ((tid & 63) == 0) {
    cnt[tid >> 6] = masked;
    flg[tid >> 6] = any;
  }
  __syncthreads();
  if (tid == 0) {
    int m = 0, a = 0;
    for (int w = 0; w < kPrepThreads / 64; ++w) {
      m += cnt[w];
      a |= flg[w];
    }
    tot[0] = m;
    tot[1] = a;
    if (A.masked_count) A.masked_count[k] = m;
  }
  __syncthreads();
  const bool stamp_flagged = tot[1] != 0;
  // pass 2: outputs (the stamp is L2-resident from pass 1)
  for (int p = tid; p < A.npix; p += kPrepThreads) {
    float d, s;
    bool flagged, both_nan;
    prep_pixel(A, k, base + p, inv_coef, t, trms2, d, s, flagged, both_nan);
    if (A.boost > 0.f && (A.boost_whole_stamp ? stamp_flagged : flagged)) s *= A.boost;
    const bool good = !(flagged || both_nan) && (d == d) && (s == s) && s > 0.f && fabsf(s) < 3.0e38f && fabsf(d) < 3.0e38f;
    if (A.data_out) A.data_out[base + p] = d;
    if (A.noisemap_out) A.noisemap_out[base + p] = s;
    if (A.weight_out) A.weight_out[base + p] = good ? 1.0f / (s * s) : 0.f;
  }
}

__global__ void copy_kernel(const float4 *src, float4 *dst, size_t n4) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) dst[i] = src[i];
}

}  // namespace lc

using namespace lc;

extern "C" {

int lc_prepare_stamps(lc_ctx *ctx, int K, int npix, const float *data, const float *noisemap, const float *rms,
                      const float *exptime, const float *coefficient, const uint8_t *bad, float nan_noise,
                      float noise_boost, int boost_whole_stamp, float *data_out, float *noisemap_out,
                      float *weight_out, int32_t *masked_count, float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  if (K <= 0 || npix <= 0 || !data) LC_FAIL(ctx, LC_ERR_INVALID, "lc_prepare_stamps: invalid argument");
  if (!noisemap && !(rms && exptime))
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_prepare_stamps: without a noise map, rms and exptime are required");
  LC_ENTER(ctx);
  const size_t tot = (size_t)K * npix;
  DeviceCall call(ctx);
  PrepArgs A;
  std::memset(&A, 0, sizeof(A));
  A.K = K;
  A.npix = npix;
  A.nan_noise = nan_noise;
  A.boost = noise_boost;
  A.boost_whole_stamp = boost_whole_stamp;
  LC_HIP(ctx, call.upload(data, tot, &A.data));
  if (noisemap) {
    LC_HIP(ctx, call.upload(noisemap, tot, &A.noisemap));
  } else {
    LC_HIP(ctx, call.upload(rms, (size_t)K, &A.rms));
    LC_HIP(ctx, call.upload(exptime, (size_t)K, &A.exptime));
  }
  LC_HIP(ctx, call.upload(coefficient, (size_t)K, &A.coefficient));
  LC_HIP(ctx, call.upload(bad, tot, &A.bad));
  LC_HIP(ctx, call.result(data_out, tot, &A.data_out));
  LC_HIP(ctx, call.result(noisemap_out, tot, &A.noisemap_out));
  LC_HIP(ctx, call.result(weight_out, tot, &A.weight_out));
  LC_HIP(ctx, call.result(masked_count, (size_t)K, &A.masked_count));
  LC_HIP(ctx, call.start());
  hipLaunchKernelGGL(prep_stamps_kernel, dim3(K), dim3(kPrepThreads), 0, ctx->stream, A);
  LC_HIP(ctx, hipGetLastError());
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

int lc_copy_bandwidth(lc_ctx *ctx, int64_t bytes, int reps, float *gb_per_s) {
  if (!ctx || !gb_per_s || bytes < 1024 || reps <= 0) return LC_ERR_INVALID;
  LC_ENTER(ctx);
  const size_t n4 = (size_t)bytes / 16;
  DevPool pool;
  float4 *a = nullptr, *b = nullptr;
  LC_HIP(ctx, pool.alloc(n4, &a));
  LC_HIP(ctx, pool.alloc(n4, &b));
  (void)hipMemsetAsync(a, 0, n4 * 16, ctx->stream);
  const int blocks = ctx->n_cu > 0 ? ctx->n_cu * 8 : 2048;
  hipLaunchKernelGGL(copy_kernel, dim3(blocks), dim3(256), 0, ctx->stream, a, b, n4);  // warm-up
  (void)hipEventRecord(ctx->ev0, ctx->stream);
  for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(copy_kernel, dim3(blocks), dim3(256), 0, ctx->stream, a, b, n4);
  (void)hipEventRecord(ctx->ev1, ctx->stream);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  if (e != hipSuccess) LC_FAIL(ctx, LC_ERR_DEVICE, std::string("lc_copy_bandwidth: ") + hipGetErrorString(e));
  *gb_per_s = (float)(2.0 * (double)n4 * 16.0 * reps / (ms * 1e-3) / 1e9);  // read + write
  return LC_OK;
}

}  // extern "C"
