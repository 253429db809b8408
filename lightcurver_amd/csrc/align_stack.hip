// Alignment and stacking of the ROI epochs: what stack_data_diagnostic (lightcurver/processes/roi_modelling.py:34-125)
// does with scipy.ndimage.shift, scipy.ndimage.rotate and a sigma-clipped weighted mean, frozen as the SPEC of
// DESIGN.md §5 "Align and stack".  Two kernels on the context's stream:
//
//   align  one workgroup per (cube, epoch), two fp32 planes in LDS (row stride n | 1: a lane per row and a lane per
//          column both walk conflict-free banks).  Cubic B-spline prefilter (a lane per line, columns then rows),
//          resample at the shift's coordinates into the second plane, prefilter again, resample at the rotation's
//          coordinates back into the first, coalesced write.  Coordinates and the in-range test in double.
//   stack  one lane per (cube, pixel), adjacent lanes adjacent pixels, so every read of an epoch is coalesced.  The
//          combine is robust_combine of order_stats.h: the median is the exact order statistic, and mean, deviation,
//          rejection and the weighted mean are sequential sums in epoch order: the result does not depend on the launch.
#pragma clang fp contract(off)  // the SPEC fixes every rounding, and the coordinates are scipy's own expressions

#include <cmath>
#include <cstring>
#include <vector>

#include "device_call.h"
#include "lc_common.h"
#include "order_stats.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kAlThreads = 256;
constexpr int kStThreads = 64;
constexpr int kAlMinN = 8, kAlMaxN = 128;
constexpr int kAlHorizon = 32;  // terms of the causal initial sum: |z|^32 = 5e-19, below the floor of either precision
constexpr int kAlGeo = 8;       // doubles per epoch: s_y, s_x, m00, m01, m10, m11, off_y, off_x

__host__ __device__ constexpr int al_ld(int n) { return n | 1; }
__host__ __device__ constexpr size_t al_lds_bytes(int n) { return (size_t)2 * n * al_ld(n) * sizeof(float); }

struct AlignArgs {
  int n;
  float pole, gain, den, last;  // z, 6, 1 - z^(2n-2), z / (z^2 - 1)
  const float *in;
  float *out;
  const double *geo;  // [E][kAlGeo]
  int E;
};

// One line of n samples, `s` floats apart: c <- its cubic B-spline coefficients (whole-sample mirror boundaries).
__device__ __forceinline__ void al_prefilter_line(float *c, int s, int n, const AlignArgs &A) {
  const float z = A.pole, g = A.gain;
  const int K = min(2 * n - 2, kAlHorizon);
  float zk = 1.0f, sum = 0.0f;
  for (int k = 0; k < K; ++k) {
    const int i = k < n ? k : 2 * n - 2 - k;
    sum = sum + zk * (g * c[i * s]);
    zk = zk * z;
  }
  float prev = sum / A.den, before = prev;
  c[0] = prev;
  for (int i = 1; i < n; ++i) {
    before = prev;
    prev = g * c[i * s] + z * prev;
    c[i * s] = prev;
  }
  float nxt = A.last * (prev + z * before);
  c[(n - 1) * s] = nxt;
  for (int i = n - 2; i >= 0; --i) {
    nxt = z * (nxt - c[i * s]);
    c[i * s] = nxt;
  }
}

__device__ __forceinline__ void al_prefilter(float *P, int n, int ld, const AlignArgs &A) {
  const int tid = threadIdx.x;
  if (tid < n) al_prefilter_line(P + tid, ld, n, A);  // column tid: lanes on adjacent banks
  __syncthreads();
  if (tid < n) al_prefilter_line(P + tid * ld, 1, n, A);  // row tid: lanes ld (odd) banks apart
  __syncthreads();
}

__device__ __forceinline__ void al_weights(float t, float w[4]) {
  const float u = 1.0f - t;
  w[1] = (t * t * (t - 2.0f) * 3.0f + 4.0f) / 6.0f;
  w[2] = (u * u * (u - 2.0f) * 3.0f + 4.0f) / 6.0f;
  w[0] = u * u * u / 6.0f;
  w[3] = 1.0f - w[0] - w[1] - w[2];
}

__device__ __forceinline__ int al_mirror(int i, int n) {
  if (i < 0) i = -i;
  if (i > n - 1) i = 2 * (n - 1) - i;
  return i;
}

// dst(y, x) = the spline with coefficients src at (m00 y + m01 x + oy, m10 y + m11 x + ox), 0 outside [0, n - 1].
__device__ __forceinline__ void al_resample(const float *src, float *dst, int n, int ld, double m00, double m01,
                                            double m10, double m11, double oy, double ox, bool diagonal) {
  const int np = n * n;
  const double hi = (double)(n - 1);
  for (int p = threadIdx.x; p < np; p += kAlThreads) {
    const int y = p / n, x = p - y * n;
    double cy, cx;
    if (diagonal) {  // scipy's shift: index + offset, per axis
      cy = (double)y + oy;
      cx = (double)x + ox;
    } else {  // scipy's affine transform: offset + sum of matrix * index, in this order
      cy = oy + (double)y * m00;
      cy = cy + (double)x * m01;
      cx = ox + (double)y * m10;
      cx = cx + (double)x * m11;
    }
    float v = 0.0f;
    if (cy >= 0.0 && cy <= hi && cx >= 0.0 && cx <= hi) {
      const double fy = floor(cy), fx = floor(cx);
      float wy[4], wx[4];
      al_weights((float)(cy - fy), wy);
      al_weights((float)(cx - fx), wx);
      const int y0 = (int)fy - 1, x0 = (int)fx - 1;
      int xi[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) xi[b] = al_mirror(x0 + b, n);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const float *row = src + al_mirror(y0 + a, n) * ld;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          float t = row[xi[b]];
          t = t * wy[a];
          t = t * wx[b];
          v = v + t;
        }
      }
    }
    dst[y * ld + x] = v;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kAlThreads) void align_kernel(AlignArgs A) {
  extern __shared__ __align__(16) float al_lds[];
  const int n = A.n, ld = al_ld(n), np = n * n, tid = threadIdx.x;
  float *P0 = al_lds, *P1 = al_lds + n * ld;
  const size_t off = (size_t)blockIdx.x * np;
  const double *g = A.geo + (size_t)(blockIdx.x % A.E) * kAlGeo;
  for (int p = tid; p < np; p += kAlThreads) {
    const int y = p / n, x = p - y * n;
    P0[y * ld + x] = A.in[off + p];
  }
  __syncthreads();
  al_prefilter(P0, n, ld, A);
  al_resample(P0, P1, n, ld, 1.0, 0.0, 0.0, 1.0, -g[0], -g[1], true);
  al_prefilter(P1, n, ld, A);
  al_resample(P1, P0, n, ld, g[2], g[3], g[4], g[5], g[6], g[7], false);
  for (int p = tid; p < np; p += kAlThreads) {
    const int y = p / n, x = p - y * n;
    A.out[off + p] = P0[y * ld + x];
  }
}

struct StackArgs {
  int E, np, clip;
  float n_sigma;
  const float *v;      // [C][E][np]
  const float *noise;  // [E][np]
  float *stack, *median;
  int32_t *nrej;
};

__global__ __launch_bounds__(kStThreads) void stack_kernel(StackArgs A) {
  const int p = blockIdx.x * kStThreads + threadIdx.x, c = blockIdx.y;
  if (p >= A.np) return;
  const size_t np = (size_t)A.np;
  const float *v = A.v + (size_t)c * A.E * np + p, *noise = A.noise + p;
  const size_t o = (size_t)c * np + p;
  const Combined r = robust_combine(
      A.E, [&](int e) { return float_key_or_missing(v[e * np]); }, [&](int e) { return 1.0f / noise[e * np]; },
      A.median || A.clip, A.clip, A.n_sigma, !A.stack && !A.nrej);
  if (A.median) A.median[o] = r.median;
  if (A.stack) A.stack[o] = r.swv / r.sw;  // NaN by 0 / 0 where no sample is finite
  if (A.nrej) A.nrej[o] = r.rej;
}

}  // namespace lc

using namespace lc;

extern "C" {

int lc_align_stack_supported(int n) { return n >= kAlMinN && n <= kAlMaxN ? 1 : 0; }

int lc_align_stack(lc_ctx *ctx, int C, int E, int n, const float *cubes, const float *noisemap, const double *shift_yx,
                   const double *angle_deg, const lc_stack_cfg *cfg, float *aligned, float *stack, float *median,
                   int32_t *n_rejected, float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  if (!lc_align_stack_supported(n)) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_align_stack: stamp size outside 8 .. 128");
  if (C < 1 || C > 65535 || E < 1 || !cubes) LC_FAIL(ctx, LC_ERR_INVALID, "lc_align_stack: invalid argument");
  if ((shift_yx == nullptr) != (angle_deg == nullptr))
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_align_stack: shift_yx and angle_deg are given or left out together");
  const bool align = shift_yx != nullptr, weighted = stack || n_rejected, stacked = weighted || median;
  if (weighted && !noisemap) LC_FAIL(ctx, LC_ERR_INVALID, "lc_align_stack: stack and n_rejected need the noise map");
  lc_stack_cfg cf = {3.0f, 1};
  if (cfg) cf = *cfg;
  if (!(cf.n_sigma > 0.f) || !std::isfinite(cf.n_sigma))
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_align_stack: n_sigma must be positive and finite");
  std::vector<double> geo;
  if (align) {
    geo.resize((size_t)E * kAlGeo);
    const double ctr = (double)(n - 1) / 2.0;
    for (int e = 0; e < E; ++e) {
      const double sy = shift_yx[2 * e], sx = shift_yx[2 * e + 1], ang = angle_deg[e];
      if (!std::isfinite(sy) || !std::isfinite(sx) || !std::isfinite(ang))
        LC_FAIL(ctx, LC_ERR_INVALID, "lc_align_stack: shifts and angles must be finite");
      const double rad = ang * (M_PI / 180.0), co = std::cos(rad), si = std::sin(rad);
      double *g = &geo[(size_t)e * kAlGeo];
      g[0] = sy;
      g[1] = sx;
      g[2] = co;
      g[3] = si;
      g[4] = -si;
      g[5] = co;
      g[6] = ctr - (co * ctr + si * ctr);
      g[7] = ctr - (-si * ctr + co * ctr);
    }
  }
  LC_ENTER(ctx);
  const size_t np = (size_t)n * n, tot = (size_t)C * E * np;
  DeviceCall call(ctx);
  const float *d_in = nullptr, *d_noise = nullptr;
  const double *d_geo = nullptr;
  float *d_al = nullptr, *d_stack = nullptr, *d_med = nullptr;
  int32_t *d_rej = nullptr;
  LC_HIP(ctx, call.upload(cubes, tot, &d_in));
  if (align) {
    LC_HIP(ctx, call.alloc(tot, &d_al));
    LC_HIP(ctx, call.upload(geo.data(), geo.size(), &d_geo));
  }
  if (weighted) LC_HIP(ctx, call.upload(noisemap, (size_t)E * np, &d_noise));
  LC_HIP(ctx, call.result(stack, (size_t)C * np, &d_stack));
  LC_HIP(ctx, call.result(median, (size_t)C * np, &d_med));
  LC_HIP(ctx, call.result(n_rejected, (size_t)C * np, &d_rej));
  const size_t lds_bytes = al_lds_bytes(n);
  if (align)
    LC_HIP(ctx, hipFuncSetAttribute((const void *)align_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes));
  LC_HIP(ctx, call.start());
  if (align) {
    const double zd = std::sqrt(3.0) - 2.0;
    AlignArgs A;
    A.n = n;
    A.pole = (float)zd;
    A.gain = 6.0f;
    A.den = (float)(1.0 - std::pow(zd, (double)(2 * n - 2)));
    A.last = (float)(zd / (zd * zd - 1.0));
    A.in = d_in;
    A.out = d_al;
    A.geo = d_geo;
    A.E = E;
    hipLaunchKernelGGL(align_kernel, dim3((unsigned)((size_t)C * E)), dim3(kAlThreads), lds_bytes, ctx->stream, A);
    LC_HIP(ctx, hipGetLastError());
  }
  const float *d_val = align ? d_al : d_in;
  if (stacked) {
    StackArgs S;
    S.E = E;
    S.np = (int)np;
    S.clip = cf.clip != 0;
    S.n_sigma = cf.n_sigma;
    S.v = d_val;
    S.noise = d_noise;
    S.stack = d_stack;
    S.median = d_med;
    S.nrej = d_rej;
    hipLaunchKernelGGL(stack_kernel, dim3((unsigned)((np + kStThreads - 1) / kStThreads), (unsigned)C), dim3(kStThreads),
                       0, ctx->stream, S);
    LC_HIP(ctx, hipGetLastError());
  }
  LC_HIP(ctx, call.stop());
  // the aligned cubes are the align kernel's work space (or, without alignment, the input): not a result() buffer
  if (aligned) LC_HIP(ctx, hipMemcpyAsync(aligned, d_val, tot * 4, hipMemcpyDeviceToHost, ctx->stream));
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

}  // extern "C"
