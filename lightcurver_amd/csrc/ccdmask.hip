// Bad rows and columns of star and ROI stamps: ccdproc's ccdmask(byblocks=False, findbadcolumns=True) and the reduction to
// whole lines that the reference's mask_cutout applies to it (lightcurver/processes/cutout_making.py:67-80), frozen as
// the SPEC of DESIGN.md §5 "Bad rows and columns".  Every float32 operation is the SPEC's, in its order; the median and
// the order statistics select values, so the masks are those of the SPEC's NumPy float32 restatement (tests/_ccdmask.py).
//
// One workgroup per stamp.  The stamp D, the residual R = D - med7x7(D) and the byte mask (9 n^2 bytes: 36 KiB at 64,
// 144 KiB at 128) live in LDS at every size.  The 49-value median is a forgetful selection in registers; the four order
// statistics of the two percentiles come from one radix select over the order-preserving integer image of R (four
// 8-bit passes, one LDS histogram per distinct prefix).  lc_mask_cutouts runs this kernel and the cosmic-ray kernel on
// one uploaded stack and returns the OR of the two masks: the whole of mask_cutout in one call.
#pragma clang fp contract(off)  // the SPEC fixes every rounding: no fused multiply-adds, on the device or the host

#include <algorithm>
#include <cstring>
#include <vector>

#include "block_reduce.h"
#include "cosmics_device.h"
#include "device_call.h"
#include "lc_common.h"
#include "mask_steps.h"
#include "order_stats.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kCmThreads = 256;  // four waves: one per order statistic in the radix select
constexpr int kCmMinN = 8, kCmMaxN = 128;
constexpr int kCmKeep = 26;  // values the forgetful selection holds at first: 49 / 2 + 2

__host__ __device__ constexpr size_t cm_lds_bytes(int n) { return (size_t)n * n * 9; }

struct CmArgs {
  int n, ngood, findbad;
  const float *data;
  uint8_t *mask, *rowcol, *bad_cols, *bad_rows;
  float *sigma;
  float lsigma, hsigma;
  int rank[4];  // ranks lo, hi of P(30.9), then lo, hi of P(69.1): ascending
  float t[2];   // the interpolation weight v - lo of P(30.9), P(69.1)
};

// scipy's 'reflect': -1 -> 0, -2 -> 1, -3 -> 2, n -> n - 1, n + 1 -> n - 2, n + 2 -> n - 3 (n >= 8: one fold is enough)
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

__device__ __forceinline__ void cmp_swap(float &a, float &b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// the smallest of v[0 .. m) to v[0], the largest to v[m - 1]
template <int m>
__device__ __forceinline__ void min_max(float (&v)[kCmKeep]) {
#pragma unroll
  for (int i = 0; i < m / 2; ++i) cmp_swap(v[i], v[m - 1 - i]);
#pragma unroll
  for (int i = 1; i < (m + 1) / 2; ++i) cmp_swap(v[0], v[i]);
#pragma unroll
  for (int i = m / 2; i < m - 1; ++i) cmp_swap(v[i], v[m - 1]);
}

// Median of the 49 window values w(0 .. 48), v holding the first 26.  Of m = (N + 3) / 2 of the N values left, neither
// the smallest nor the largest can be the median of the N: both are dropped and the next value takes a place, until
// three are left.  522 compare-exchanges (a counting selection costs 49^2 = 2401 compare pairs).
template <int m, class W>
__device__ __forceinline__ float forget_select(float (&v)[kCmKeep], const W &w) {
  min_max<m>(v);
  if constexpr (m > 3) {
    v[0] = w(kCmKeep + (kCmKeep - m));
    return forget_select<m - 1>(v, w);
  } else {
    return v[1];
  }
}

// NumPy's linear interpolation between the order statistics a (rank lo) and b (rank hi)
__device__ __forceinline__ float interpolate(float a, float b, float t) {
  const float d = b - a;
  return t >= 0.5f ? b - d * (1.0f - t) : a + d * t;
}

__global__ __launch_bounds__(kCmThreads) void ccdmask_kernel(CmArgs A) {
  extern __shared__ __align__(16) float cm_lds[];
  __shared__ unsigned s_hist[4][256];
  __shared__ unsigned s_prefix[4];
  __shared__ int s_rank[4], s_own[4];
  __shared__ float s_sigma;
  __shared__ uint8_t s_bc[kCmMaxN], s_br[kCmMaxN];
  const int n = A.n, np = n * n, tid = threadIdx.x, k = blockIdx.x;
  float *D = cm_lds, *R = D + np;
  uint8_t *M = (uint8_t *)(R + np);
  const size_t off = (size_t)k * np;

  // 1: M = ~isfinite(D); any such pixel makes sigma NaN, and steps 2 - 4 then add nothing
  int holes = 0;
  for (int p = tid; p < np; p += kCmThreads) {
    const float d = A.data[off + p];
    const bool h = !__builtin_isfinite(d);
    D[p] = d;
    M[p] = h ? 1 : 0;
    holes |= h;
  }
  if (tid == 0) s_sigma = __builtin_nanf("");
  if (!__syncthreads_or(holes)) {
    // 2: R = D - med7x7(D)
    for (int p = tid; p < np; p += kCmThreads) {
      const int i = p / n, j = p - i * n;
      int ro[7], co[7];
#pragma unroll
      for (int a = 0; a < 7; ++a) {
        ro[a] = reflect(i - 3 + a, n) * n;
        co[a] = reflect(j - 3 + a, n);
      }
      const auto w = [&](int a) { return D[ro[a / 7] + co[a % 7]]; };
      float v[kCmKeep];
#pragma unroll
      for (int a = 0; a < kCmKeep; ++a) v[a] = w(a);
      R[p] = D[p] - forget_select<kCmKeep>(v, w);
    }
    if (tid < 4) {
      s_prefix[tid] = 0;
      s_rank[tid] = A.rank[tid];
    }
    __syncthreads();
    // 3: the four order statistics of R by radix select, most significant byte first.  Rank r counts the keys that
    // carry its prefix; ranks with the same prefix share the histogram of the first of them (s_own).
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      const unsigned high = pass ? 0xFFFFFFFFu << (shift + 8) : 0u;
      if (tid < 4) {
        int own = tid;
        while (own > 0 && s_prefix[own - 1] == s_prefix[tid]) --own;
        s_own[tid] = own;
      }
      for (int b = tid; b < 4 * 256; b += kCmThreads) (&s_hist[0][0])[b] = 0;
      __syncthreads();
      unsigned pf[4];
      bool owner[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pf[r] = s_prefix[r];
        owner[r] = s_own[r] == r;
      }
      for (int p = tid; p < np; p += kCmThreads) {
        const unsigned key = float_key(R[p]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (owner[r] && (key & high) == pf[r]) atomicAdd(&s_hist[r][(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      {
        // wave r finds the bin of rank r: lane l holds bins 4 l .. 4 l + 3, an inclusive scan over the lanes
        const int r = tid >> 6, lane = tid & 63;
        const unsigned *h = s_hist[s_own[r]];
        int want = s_rank[r];
        const int c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2], c3 = h[4 * lane + 3];
        const int mine = (c0 + c1) + (c2 + c3);
        const int incl = wave_inclusive_scan(mine);
        const int excl = incl - mine;
        if (excl <= want && want < incl) {
          want -= excl;
          int bin = 4 * lane;
          if (want >= c0) {
            want -= c0;
            ++bin;
            if (want >= c1) {
              want -= c1;
              ++bin;
              if (want >= c2) {
                want -= c2;
                ++bin;
              }
            }
          }
          s_prefix[r] |= (unsigned)bin << shift;
          s_rank[r] = want;
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      const float p_lo = interpolate(float_unkey(s_prefix[0]), float_unkey(s_prefix[1]), A.t[0]);
      const float p_hi = interpolate(float_unkey(s_prefix[2]), float_unkey(s_prefix[3]), A.t[1]);
      s_sigma = (p_hi - p_lo) / 2.0f;
    }
    __syncthreads();
    // 4: the threshold
    const float below = -(A.lsigma * s_sigma), above = A.hsigma * s_sigma;
    for (int p = tid; p < np; p += kCmThreads) {
      const float r = R[p];
      if (r < below || r > above) M[p] = 1;
    }
    __syncthreads();
  }
  // 5: short gaps along columns, in place and in order: one lane walks down each column
  if (A.findbad && tid < n) {
    for (int line = 0; line <= n - A.ngood - 2; ++line) {
      if (!M[line * n + tid]) continue;
      for (int i = 2; i <= A.ngood + 1; ++i)
        if (M[(line + i) * n + tid])
          for (int q = line + 1; q < line + i; ++q) M[q * n + tid] = 1;
    }
  }
  __syncthreads();
  // 6: lines that reach both ends of the stamp
  if (tid < n) {
    s_bc[tid] = M[tid] & M[(n - 1) * n + tid];
    s_br[tid] = M[tid * n] & M[tid * n + n - 1];
  }
  __syncthreads();
  for (int p = tid; p < np; p += kCmThreads) {
    const int i = p / n, j = p - i * n;
    if (A.mask) A.mask[off + p] = M[p];
    if (A.rowcol) A.rowcol[off + p] = s_bc[j] | s_br[i];
  }
  if (tid < n) {
    if (A.bad_cols) A.bad_cols[(size_t)k * n + tid] = s_bc[tid];
    if (A.bad_rows) A.bad_rows[(size_t)k * n + tid] = s_br[tid];
  }
  if (tid == 0 && A.sigma) A.sigma[k] = s_sigma;
}

__global__ __launch_bounds__(256) void square_kernel(const float *x, float *y, size_t count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) y[i] = x[i] * x[i];
}

__global__ __launch_bounds__(256) void or_kernel(uint8_t *a, const uint8_t *b, size_t count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) a[i] |= b[i];
}

int ccdmask_check(lc_ctx *ctx, const char *who, int n, const lc_ccdmask_cfg *cfg) {
  const std::string w(who);
  if (n < kCmMinN || n > kCmMaxN) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, w + ": stamp size outside 8 .. 128");
  if (cfg->byblocks != 0) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, w + ": byblocks is not built");
  if (cfg->ncmed != 7 || cfg->nlmed != 7) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, w + ": only the 7 x 7 median window is built");
  if (!std::isfinite(cfg->lsigma) || !std::isfinite(cfg->hsigma) || cfg->ngood < 0)
    LC_FAIL(ctx, LC_ERR_INVALID, w + ": invalid settings");
  return LC_OK;
}

// rank lo, rank hi and weight t = v - lo of NumPy's linear percentile p over count values
static void percentile_ranks(float p, int count, int *lo, int *hi, float *t) {
  const float q = p / 100.0f;
  const float v = (float)(count - 1) * q;
  *lo = (int)std::floor(v);
  *hi = std::min(*lo + 1, count - 1);
  *t = v - (float)*lo;
}

// one launch on ctx->stream over K stamps; every pointer is a device pointer, any output may be null
hipError_t ccdmask_launch(lc_ctx *ctx, int K, int n, const float *data, const lc_ccdmask_cfg *cfg, uint8_t *mask,
                          uint8_t *rowcol, uint8_t *bad_cols, uint8_t *bad_rows, float *sigma) {
  CmArgs A;
  std::memset(&A, 0, sizeof(A));
  A.n = n;
  A.ngood = std::min(cfg->ngood, n);  // from n - 1 on no line can start a fill
  A.findbad = cfg->findbadcolumns != 0;
  A.data = data;
  A.mask = mask;
  A.rowcol = rowcol;
  A.bad_cols = bad_cols;
  A.bad_rows = bad_rows;
  A.sigma = sigma;
  A.lsigma = cfg->lsigma;
  A.hsigma = cfg->hsigma;
  percentile_ranks(30.9f, n * n, &A.rank[0], &A.rank[1], &A.t[0]);
  percentile_ranks(69.1f, n * n, &A.rank[2], &A.rank[3], &A.t[1]);
  const size_t lds_bytes = cm_lds_bytes(n);
  hipError_t e = hipFuncSetAttribute((const void *)ccdmask_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ccdmask_kernel, dim3(K), dim3(kCmThreads), lds_bytes, ctx->stream, A);
  return hipGetLastError();
}

hipError_t square_launch(lc_ctx *ctx, const float *x, float *y, size_t count) {
  hipLaunchKernelGGL(square_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, x, y, count);
  return hipGetLastError();
}

hipError_t or_launch(lc_ctx *ctx, uint8_t *a, const uint8_t *b, size_t count) {
  hipLaunchKernelGGL(or_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, a, b, count);
  return hipGetLastError();
}

hipError_t mask_cutouts_scratch(DeviceCall &call, const lc_ctx *ctx, int K, int n, int do_bad_columns, int do_cosmics,
                                MaskCutoutsScratch *S) {
  if (!do_cosmics) return hipSuccess;
  const size_t tot = (size_t)K * n * n;
  hipError_t e = call.alloc(tot, &S->invar);
  if (e != hipSuccess) return e;
  if (const size_t sb = cosmics_scratch_bytes(ctx, K, n))
    if ((e = call.alloc(sb / 4, &S->cosmics)) != hipSuccess) return e;
  return do_bad_columns ? call.alloc(tot, &S->lines) : hipSuccess;
}

hipError_t mask_cutouts_launch(lc_ctx *ctx, int K, int n, const float *data, const float *noisemap, int do_bad_columns,
                               int do_cosmics, const lc_cosmics_cfg *cosmics_cfg, const lc_ccdmask_cfg *ccdmask_cfg,
                               const MaskCutoutsScratch &S, uint8_t *mask) {
  const size_t tot = (size_t)K * n * n;
  hipError_t e = hipSuccess;
  if (do_cosmics) {
    if ((e = square_launch(ctx, noisemap, S.invar, tot)) != hipSuccess) return e;
    e = cosmics_launch(ctx, K, n, data, S.invar, nullptr, cosmics_cfg, mask, nullptr, nullptr, S.cosmics);
    if (e != hipSuccess) return e;
  }
  if (do_bad_columns) {
    uint8_t *rowcol = do_cosmics ? S.lines : mask;
    if ((e = ccdmask_launch(ctx, K, n, data, ccdmask_cfg, nullptr, rowcol, nullptr, nullptr, nullptr)) != hipSuccess) return e;
    if (do_cosmics) e = or_launch(ctx, mask, S.lines, tot);
  }
  return e;
}

}  // namespace lc

using namespace lc;

extern "C" {

int lc_ccdmask_supported(int n) { return n >= kCmMinN && n <= kCmMaxN ? 1 : 0; }

int lc_ccdmask_stamps(lc_ctx *ctx, int K, int n, const float *data, const lc_ccdmask_cfg *cfg, uint8_t *mask,
                      uint8_t *rowcol, uint8_t *bad_cols, uint8_t *bad_rows, float *sigma, float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  if (K <= 0 || !data || !cfg || !(mask || rowcol || bad_cols || bad_rows || sigma))
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_ccdmask_stamps: invalid argument");
  if (int rc = ccdmask_check(ctx, "lc_ccdmask_stamps", n, cfg)) return rc;
  LC_ENTER(ctx);
  const size_t np = (size_t)n * n, tot = (size_t)K * np, lines = (size_t)K * n;
  DeviceCall call(ctx);
  const float *d_data = nullptr;
  float *d_sigma = nullptr;
  uint8_t *d_mask = nullptr, *d_rowcol = nullptr, *d_cols = nullptr, *d_rows = nullptr;
  LC_HIP(ctx, call.upload(data, tot, &d_data));
  LC_HIP(ctx, call.result(mask, tot, &d_mask));
  LC_HIP(ctx, call.result(rowcol, tot, &d_rowcol));
  LC_HIP(ctx, call.result(bad_cols, lines, &d_cols));
  LC_HIP(ctx, call.result(bad_rows, lines, &d_rows));
  LC_HIP(ctx, call.result(sigma, (size_t)K, &d_sigma));
  LC_HIP(ctx, call.start());
  LC_HIP(ctx, ccdmask_launch(ctx, K, n, d_data, cfg, d_mask, d_rowcol, d_cols, d_rows, d_sigma));
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

int lc_mask_cutouts(lc_ctx *ctx, int K, int n, const float *data, const float *noisemap, int do_bad_columns,
                    int do_cosmics, const lc_cosmics_cfg *cosmics_cfg, const lc_ccdmask_cfg *ccdmask_cfg, uint8_t *mask,
                    float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  if (K <= 0 || !data || !mask || (do_cosmics && (!noisemap || !cosmics_cfg)) || (do_bad_columns && !ccdmask_cfg))
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_mask_cutouts: invalid argument");
  if (do_cosmics)
    if (int rc = cosmics_check(ctx, "lc_mask_cutouts", n, cosmics_cfg)) return rc;
  if (do_bad_columns)
    if (int rc = ccdmask_check(ctx, "lc_mask_cutouts", n, ccdmask_cfg)) return rc;
  const size_t np = (size_t)n * n, tot = (size_t)K * np;
  if (!do_cosmics && !do_bad_columns) {
    std::memset(mask, 0, tot);
    if (kernel_ms) *kernel_ms = 0.f;
    return LC_OK;
  }
  LC_ENTER(ctx);
  DeviceCall call(ctx);
  const float *d_data = nullptr;
  uint8_t *d_mask = nullptr;
  MaskCutoutsScratch S;
  LC_HIP(ctx, call.upload(data, tot, &d_data));
  LC_HIP(ctx, call.result(mask, tot, &d_mask));
  LC_HIP(ctx, mask_cutouts_scratch(call, ctx, K, n, do_bad_columns, do_cosmics, &S));
  if (do_cosmics)  // the noise map goes where it is squared in place: not upload()'s read-only input
    LC_HIP(ctx, hipMemcpyAsync(S.invar, noisemap, tot * 4, hipMemcpyHostToDevice, ctx->stream));
  LC_HIP(ctx, call.start());
  LC_HIP(ctx, mask_cutouts_launch(ctx, K, n, d_data, S.invar, do_bad_columns, do_cosmics, cosmics_cfg, ccdmask_cfg, S, d_mask));
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

}  // extern "C"
