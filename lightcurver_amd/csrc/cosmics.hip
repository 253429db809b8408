// Cosmic-ray detection on star and ROI stamps: L.A.Cosmic (van Dokkum 2001) as astroscrappy's detect_cosmics applies it
// with the reference's arguments (lightcurver/processes/cutout_making.py:85, config.yaml:209-214), frozen as the SPEC of
// DESIGN.md §5 "Cosmic-ray detection".  Every float32 operation is the SPEC's, in its order; the medians select values,
// so the result is bit for bit that of the SPEC's NumPy float32 restatement (tests/_lacosmic.py).
//
// One workgroup per stamp, every niter iteration inside the launch, the early exit a workgroup-wide vote.  The stamp's
// planes (C, N, SP, F, two temporaries, four byte masks: 28 n^2 bytes) live in LDS up to n = 64 (112 KiB) and in a
// global scratch slab per workgroup above that (the grid then strides over the stamps).  Separable medians of 5, 7 and
// 9 values are sorted in registers by transposition networks; the 9-, 25- and 49-value medians of sepmed = 0 are
// counting selections over the window.
#pragma clang fp contract(off)  // the SPEC fixes every rounding: no fused multiply-adds, on the device or the host

#include <algorithm>
#include <cstring>
#include <vector>

#include "block_reduce.h"
#include "cosmics_device.h"
#include "device_call.h"
#include "lacosmic_steps.h"
#include "lc_common.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kCrThreads = 256;
constexpr int kCrMinN = 8, kCrMaxN = 128, kCrLdsMaxN = 64;
constexpr int kCrFloatPlanes = 6, kCrBytePlanes = 4;

__host__ __device__ constexpr size_t cr_plane_bytes(int n) {
  return (size_t)n * n * (4 * kCrFloatPlanes + kCrBytePlanes);
}

struct CrArgs {
  int K, n, niter, sepmed, have_invar;
  const float *data, *invar;
  const uint8_t *inmask;
  uint8_t *crmask;
  float *clean;
  int *iters;
  float *scratch;       // global planes (n > kCrLdsMaxN): gridDim.x slabs of cr_plane_bytes(n)
  float gain, gain2;    // gain, gain * gain
  float rn2, vhole;     // readnoise^2, 1e-5 + readnoise^2 (the variance the NaN rule gives a hole)
  float satg, satg10;   // gain * satlevel, (gain * satlevel) / 10
  float sigclip, sigcliplow, objlim;  // sigcliplow = sigfrac * sigclip
};

// full k x k median by counting selection (rank (k*k)/2): the sepmed = 0 path, correct rather than fast
__device__ __forceinline__ void med_full(const float *X, float *Y, int n, int k) {
  const int h = k / 2, np = n * n, r = (k * k) / 2;
  for (int p = threadIdx.x; p < np; p += kCrThreads) {
    const int i = p / n, j = p - i * n;
    if (i < h || i >= n - h || j < h || j >= n - h) {
      Y[p] = X[p];
      continue;
    }
    float out = X[p];
    for (int a = 0; a < k * k; ++a) {
      const float va = X[(i - h + a / k) * n + (j - h + a % k)];
      int less = 0, le = 0;
      for (int b = 0; b < k * k; ++b) {
        const float vb = X[(i - h + b / k) * n + (j - h + b % k)];
        less += vb < va;
        le += vb <= va;
      }
      if (less <= r && r < le) {
        out = va;
        break;
      }
    }
    Y[p] = out;
  }
}

// Y = median of X: sepmed -> 1 x KS then KS x 1 (T is the row pass's output), else the full k_full x k_full median
template <int KS>
__device__ __forceinline__ void median(bool sepmed, int k_full, const float *X, float *T, float *Y, int n) {
  if (sepmed) {
    la_sep_median<KS, kCrThreads>(X, T, Y, n, LaRegion{0, 0, n, n});
  } else {
    med_full(X, Y, n, k_full);
    __syncthreads();
  }
}

template <bool kLds>
__global__ __launch_bounds__(kCrThreads) void cosmics_kernel(CrArgs A) {
  extern __shared__ __align__(16) float cr_lds[];
  __shared__ int s_cnt[kCrThreads / kWave];
  __shared__ float s_fallback;
  const int n = A.n, np = n * n, tid = threadIdx.x;
  const bool sepmed = A.sepmed != 0;
  const LaRegion stamp = {0, 0, n, n};  // the region of lacosmic_steps.h is the whole stamp
  float *base = kLds ? cr_lds : A.scratch + (size_t)blockIdx.x * (cr_plane_bytes(n) / 4);
  float *C = base, *Np = C + np, *S = Np + np, *T1 = S + np, *T2 = T1 + np, *Fp = T2 + np;
  uint8_t *M = (uint8_t *)(Fp + np), *CR = M + np, *B1 = CR + np, *B2 = B1 + np;

  for (int k = blockIdx.x; k < A.K; k += gridDim.x) {
    const size_t off = (size_t)k * np;
    // 0: C = gain D, V = invar gain^2, mask = inmask + the NaN rule
    for (int p = tid; p < np; p += kCrThreads) {
      float c, nz;
      bool m;
      la_input(A.data[off + p], A.have_invar, A.have_invar ? A.invar[off + p] : 0.f, A.inmask && A.inmask[off + p] != 0,
               A.gain, A.gain2, A.vhole, &c, &nz, &m);
      C[p] = c;
      if (A.have_invar) Np[p] = nz;
      M[p] = m ? 1 : 0;
      CR[p] = 0;
    }
    __syncthreads();
    // 1: saturated pixels, grown by two 3 x 3 dilations
    median<7>(sepmed, 5, C, T1, T2, n);
    for (int p = tid; p < np; p += kCrThreads) B1[p] = (C[p] >= A.satg && T2[p] > A.satg10) ? 1 : 0;
    __syncthreads();
    for (int p = tid; p < np; p += kCrThreads) B2[p] = la_dil3(B1, p / n, p % n, n) ? 1 : 0;
    __syncthreads();
    for (int p = tid; p < np; p += kCrThreads) M[p] |= la_dil3(B2, p / n, p % n, n) ? 1 : 0;
    __syncthreads();

    int done = 0;
    for (int it = 0; it < A.niter; ++it) {
      done = it + 1;
      // b: noise model without invar
      if (!A.have_invar) {
        median<7>(sepmed, 5, C, T1, T2, n);
        for (int p = tid; p < np; p += kCrThreads) Np[p] = sqrtf(fmaxf(T2[p], 1e-5f) + A.rn2);
        __syncthreads();
      }
      // a, c: S = L / (2 N), SP = S - m5(S)
      for (int p = tid; p < np; p += kCrThreads) {
        const int i = p / n, j = p - i * n;
        S[p] = la_laplace(C, i, j, n, stamp) / (2.0f * Np[p]);
      }
      __syncthreads();
      median<7>(sepmed, 5, S, T1, T2, n);
      for (int p = tid; p < np; p += kCrThreads) S[p] = S[p] - T2[p];
      // d: fine structure F = max((m3 - m7(m3)) / N, 0.01)
      median<5>(sepmed, 3, C, T1, Fp, n);
      median<9>(sepmed, 7, Fp, T1, T2, n);
      for (int p = tid; p < np; p += kCrThreads) Fp[p] = fmaxf((Fp[p] - T2[p]) / Np[p], 0.01f);
      __syncthreads();
      // e, f: candidates and their growth
      for (int p = tid; p < np; p += kCrThreads) {
        const float sp = S[p];
        B1[p] = (sp > A.sigclip && !M[p] && sp / Fp[p] > A.objlim) ? 1 : 0;
      }
      __syncthreads();
      for (int p = tid; p < np; p += kCrThreads)
        B2[p] = (la_dil3(B1, p / n, p % n, n) && S[p] > A.sigclip && !M[p]) ? 1 : 0;
      __syncthreads();
      // g: CR |= g2; stop when g2 is empty
      int any = 0;
      for (int p = tid; p < np; p += kCrThreads) {
        if (la_dil3(B2, p / n, p % n, n) && S[p] > A.sigcliplow && !M[p]) {
          CR[p] = 1;
          any = 1;
        }
      }
      if (!__syncthreads_or(any)) break;
      // h: meanmask from the C of before this step; T1 = replacement, B1 = no good pixel in the window
      int need = 0;
      for (int p = tid; p < np; p += kCrThreads) {
        if (!CR[p]) continue;
        const int i = p / n, j = p - i * n;
        float acc = 0.f;
        int cnt = 0;
        for (int y = max(i - 2, 0); y <= min(i + 2, n - 1); ++y)
          for (int x = max(j - 2, 0); x <= min(j + 2, n - 1); ++x) {
            const int q = y * n + x;
            if (!CR[q] && !M[q]) {
              acc = acc + C[q];
              ++cnt;
            }
          }
        B1[p] = cnt == 0 ? 1 : 0;
        if (cnt) T1[p] = acc / (float)cnt;
        need |= cnt == 0;
      }
      if (__syncthreads_or(need)) {
        // lower median (rank (m - 1) / 2) of the good pixels of the stamp, by counting; 0 when there are none
        int m = 0;
        for (int p = tid; p < np; p += kCrThreads) m += (!CR[p] && !M[p]) ? 1 : 0;
        if (tid == 0) s_fallback = 0.f;
        m = block_sum<kCrThreads / kWave>(m, s_cnt);
        const int r = (m - 1) / 2;
        for (int p = tid; p < np && m > 0; p += kCrThreads) {
          if (CR[p] || M[p]) continue;
          const float va = C[p];
          int less = 0, le = 0;
          for (int q = 0; q < np; ++q) {
            if (CR[q] || M[q]) continue;
            less += C[q] < va;
            le += C[q] <= va;
          }
          if (less <= r && r < le) s_fallback = va;  // every writer holds the same value
        }
        __syncthreads();
      }
      for (int p = tid; p < np; p += kCrThreads)
        if (CR[p]) C[p] = B1[p] ? s_fallback : T1[p];
      __syncthreads();
    }
    for (int p = tid; p < np; p += kCrThreads) {
      A.crmask[off + p] = CR[p];
      if (A.clean) A.clean[off + p] = C[p] / A.gain;
    }
    if (tid == 0 && A.iters) A.iters[k] = done;
    __syncthreads();  // the planes are reused by the next stamp of this workgroup
  }
}

int cosmics_check(lc_ctx *ctx, const char *who, int n, const lc_cosmics_cfg *cfg) {
  const std::string w(who);
  if (n < kCrMinN || n > kCrMaxN) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, w + ": stamp size outside 8 .. 128");
  if (cfg->cleantype != 0 || cfg->fsmode != 0)
    LC_FAIL(ctx, LC_ERR_UNSUPPORTED, w + ": only cleantype = meanmask and fsmode = median are built");
  if (!(cfg->gain > 0.f) || !std::isfinite(cfg->gain) || !std::isfinite(cfg->readnoise) ||
      !std::isfinite(cfg->sigclip) || !std::isfinite(cfg->sigfrac) || !std::isfinite(cfg->objlim) ||
      std::isnan(cfg->satlevel) || cfg->niter < 0)
    LC_FAIL(ctx, LC_ERR_INVALID, w + ": invalid settings");
  return LC_OK;
}

static int cosmics_grid(const lc_ctx *ctx, int K, int n) {
  return n <= kCrLdsMaxN ? K : std::min(K, std::max(ctx->n_cu, 1) * 2);
}

size_t cosmics_scratch_bytes(const lc_ctx *ctx, int K, int n) {
  return n <= kCrLdsMaxN ? 0 : (size_t)cosmics_grid(ctx, K, n) * cr_plane_bytes(n);
}

hipError_t cosmics_launch(lc_ctx *ctx, int K, int n, const float *data, const float *invar, const uint8_t *inmask,
                          const lc_cosmics_cfg *cfg, uint8_t *crmask, float *clean, int32_t *iters, float *scratch) {
  CrArgs A;
  std::memset(&A, 0, sizeof(A));
  A.K = K;
  A.n = n;
  A.niter = cfg->niter;
  A.sepmed = cfg->sepmed != 0;
  A.have_invar = invar != nullptr;
  A.data = data;
  A.invar = invar;
  A.inmask = inmask;
  A.crmask = crmask;
  A.clean = clean;
  A.iters = iters;
  A.scratch = scratch;
  A.gain = cfg->gain;
  A.gain2 = cfg->gain * cfg->gain;
  A.rn2 = cfg->readnoise * cfg->readnoise;
  A.vhole = 1e-5f + A.rn2;
  A.satg = cfg->gain * cfg->satlevel;
  A.satg10 = A.satg / 10.0f;
  A.sigclip = cfg->sigclip;
  A.sigcliplow = cfg->sigfrac * cfg->sigclip;
  A.objlim = cfg->objlim;
  const int grid = cosmics_grid(ctx, K, n);
  if (n <= kCrLdsMaxN) {
    const size_t lds_bytes = cr_plane_bytes(n);
    hipError_t e = hipFuncSetAttribute((const void *)cosmics_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cosmics_kernel<true>, dim3(grid), dim3(kCrThreads), lds_bytes, ctx->stream, A);
  } else {
    hipLaunchKernelGGL(cosmics_kernel<false>, dim3(grid), dim3(kCrThreads), 0, ctx->stream, A);
  }
  return hipGetLastError();
}

}  // namespace lc

using namespace lc;

extern "C" {

int lc_cosmics_supported(int n) { return n >= kCrMinN && n <= kCrMaxN ? 1 : 0; }

int lc_detect_cosmics(lc_ctx *ctx, int K, int n, const float *data, const float *invar, const uint8_t *inmask,
                      const lc_cosmics_cfg *cfg, uint8_t *crmask, float *clean, int32_t *iters, float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  if (K <= 0 || !data || !cfg || !crmask) LC_FAIL(ctx, LC_ERR_INVALID, "lc_detect_cosmics: invalid argument");
  if (int rc = cosmics_check(ctx, "lc_detect_cosmics", n, cfg)) return rc;
  LC_ENTER(ctx);
  const size_t np = (size_t)n * n, tot = (size_t)K * np;
  DeviceCall call(ctx);
  const float *d_data = nullptr, *d_invar = nullptr;
  const uint8_t *d_inmask = nullptr;
  uint8_t *d_crmask = nullptr;
  float *d_clean = nullptr, *d_scratch = nullptr;
  int32_t *d_iters = nullptr;
  LC_HIP(ctx, call.upload(data, tot, &d_data));
  LC_HIP(ctx, call.upload(invar, tot, &d_invar));
  LC_HIP(ctx, call.upload(inmask, tot, &d_inmask));
  LC_HIP(ctx, call.result(crmask, tot, &d_crmask));
  LC_HIP(ctx, call.result(clean, tot, &d_clean));
  LC_HIP(ctx, call.result(iters, (size_t)K, &d_iters));
  if (const size_t sb = cosmics_scratch_bytes(ctx, K, n)) LC_HIP(ctx, call.alloc(sb / 4, &d_scratch));
  LC_HIP(ctx, call.start());
  LC_HIP(ctx, cosmics_launch(ctx, K, n, d_data, d_invar, d_inmask, cfg, d_crmask, d_clean, d_iters, d_scratch));
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

}  // extern "C"
