// Co-addition of whole frames: the registered frames of a resident set resampled onto one grid in reference pixels and
// combined, frozen as the SPEC of DESIGN.md §5 "Co-addition of frames".  Strip by strip over the output rows, two
// kernels per strip on the context's stream:
//
//   warp     one lane per (frame of the list, output pixel of the strip), adjacent lanes adjacent output pixels, so the
//            gathers of a nearly aligned frame are nearly coalesced and the write is.  Coordinates, floor and the
//            all-taps-inside test in double; weights and the tap sum in float32, y-major.  Writes the samples [n][rows][W]
//            to scratch, NaN where a tap falls outside the frame.
//   combine  one lane per output pixel, adjacent lanes adjacent pixels, so every read of a frame's samples is coalesced.
//            The combine is robust_combine of order_stats.h, which stack_kernel (align_stack.hip) calls too: the median
//            is the exact order statistic, both middle elements at once.  Every sum runs in the order of the list: the
//            result depends neither on the launch shape nor on the strip height.  The samples of a pixel are read 35
//            times (count, 32 bisection steps, deviation, weighted mean): up to kCoLdsFrames frames a wave first copies
//            the keys of its n x 64 samples to LDS (lane-major: conflict-free) and makes the passes there; beyond that
//            the passes read the scratch.  Both forms run the same arithmetic in the same order.
#pragma clang fp contract(off)  // the SPEC fixes every rounding

#include <cmath>
#include <cstring>
#include <vector>

#include "device_call.h"
#include "frames_state.h"
#include "lc_common.h"
#include "order_stats.h"
#include "resample_device.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kCoThreads = 256;
constexpr int kCoLdsThreads = kWave;                   // the combine with its samples in LDS: one wave per workgroup
constexpr int kCoLdsFrames = 160 * 1024 / (kCoLdsThreads * (int)sizeof(float));  // 640: what the LDS of a CU holds
constexpr size_t kCoScratchBytes = (size_t)128 << 20;  // the strip height is the most rows whose samples fit this

struct CoaddWarpArgs {
  int n, rows, W, h, w, order;
  int x0, row0;           // reference pixel of the strip's first sample: (x0 + j, row0 + r)
  const float *planes;    // [K][h][w]
  const int32_t *frame;   // [n]
  const double *affine;   // [n][6]
  const float *scale;     // [n]: float32(g |det A|)
  float *samples;         // [n][rows][W]
};

__global__ __launch_bounds__(kCoThreads) void coadd_warp_kernel(CoaddWarpArgs A) {
  const int tiles = (A.W + kCoThreads - 1) / kCoThreads;
  const size_t b = blockIdx.x;
  const int tile = (int)(b % tiles);
  const size_t kr = b / tiles;
  const int r = (int)(kr % A.rows), k = (int)(kr / A.rows);
  const int j = tile * kCoThreads + threadIdx.x;
  if (j >= A.W || k >= A.n) return;
  const double *M = A.affine + (size_t)k * 6;
  const float v = co_resample(A.planes + (size_t)A.frame[k] * A.h * A.w, A.h, A.w, M, (double)(A.x0 + j),
                              (double)(A.row0 + r), A.order, A.scale[k]);
  A.samples[((size_t)k * A.rows + r) * A.W + j] = v;
}

struct CoaddCombineArgs {
  int n, combine;
  size_t np, stride;      // pixels of the strip, and the samples of one frame (= np)
  float n_sigma;
  const float *samples;   // [n][np]
  const float *weight;    // [n]
  float *image, *wsum;    // [np] at the strip's first pixel; wsum, count, nrej nullable
  int32_t *count, *nrej;
};

// LDS: the keys of the wave's samples [n][64] are written to LDS first and every pass reads them there; the passes that
// need the value take it back from the key, which is exact
template <bool LDS>
__global__ __launch_bounds__(LDS ? kCoLdsThreads : kCoThreads) void coadd_combine_kernel(CoaddCombineArgs A) {
  extern __shared__ __align__(16) unsigned co_lds[];
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= A.np) return;  // (no barrier follows: a lane reads back only what it wrote)
  const int n = A.n;
  const float *v = A.samples + p;
  const size_t st = A.stride;
  unsigned *mine = co_lds + threadIdx.x;
  if (LDS)
    for (int k = 0; k < n; ++k) mine[k * kCoLdsThreads] = float_key_or_missing(v[k * st]);
  const Combined r = robust_combine(
      n, [&](int k) { return LDS ? mine[k * kCoLdsThreads] : float_key_or_missing(v[k * st]); },
      [&](int k) { return A.weight[k]; }, A.combine != LC_COADD_MEAN, A.combine == LC_COADD_SIGMA_CLIP, A.n_sigma, false);
  A.image[p] = r.m == 0 ? __builtin_nanf("") : A.combine == LC_COADD_MEDIAN ? r.median : r.swv / r.sw;
  if (A.wsum) A.wsum[p] = r.sw;
  if (A.count) A.count[p] = r.kept;
  if (A.nrej) A.nrej[p] = r.rej;
}

}  // namespace lc

using namespace lc;

extern "C" {

int lc_frames_coadd(lc_frames *f, int n, const int32_t *frame, const double *affine, const float *flux_scale,
                    const float *weight, int H, int W, int x0, int y0, const lc_coadd_cfg *cfg, float *image,
                    float *weight_out, int32_t *count, int32_t *n_rejected, float *kernel_ms) {
  if (!f) return LC_ERR_INVALID;
  lc_ctx *ctx = f->ctx;
  if (n < 1 || !frame || !affine || !cfg || !image) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_coadd: invalid argument");
  if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31))
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_coadd: H and W must be >= 1 with H W < 2^31");
  // (the grid's last reference pixel must be an int: x0 + W - 1, y0 + H - 1)
  if ((int64_t)x0 + W > INT32_MAX || (int64_t)y0 + H > INT32_MAX)
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_coadd: the grid leaves the range of int");
  if (cfg->order != 1 && cfg->order != 3) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_coadd: order must be 1 or 3");
  if (cfg->combine != LC_COADD_MEAN && cfg->combine != LC_COADD_MEDIAN && cfg->combine != LC_COADD_SIGMA_CLIP)
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_coadd: unknown combine");
  if (!(cfg->n_sigma > 0.f) || !std::isfinite(cfg->n_sigma))
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_coadd: n_sigma must be positive and finite");
  if (cfg->scratch_rows < 0) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_coadd: scratch_rows must be >= 0");
  std::vector<float> scale((size_t)n), wt((size_t)n, 1.0f);
  for (int k = 0; k < n; ++k) {
    if (frame[k] < 0 || frame[k] >= f->K) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_coadd: a frame index outside the set");
    const double *M = affine + (size_t)k * 6;
    for (int i = 0; i < 6; ++i)
      if (!std::isfinite(M[i])) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_coadd: an affine entry that is not finite");
    const double det = M[0] * M[4] - M[1] * M[3];
    if (det == 0.0 || !std::isfinite(det)) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_coadd: an affine without an inverse");
    const double g = flux_scale ? (double)flux_scale[k] : 1.0;
    if (!std::isfinite(g)) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_coadd: a flux scale that is not finite");
    scale[k] = (float)(g * std::fabs(det));
    if (!std::isfinite(scale[k])) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_coadd: a flux scale that is not finite");
    if (weight) {
      if (!std::isfinite(weight[k]) || weight[k] < 0.0f)
        LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_coadd: a weight that is negative or not finite");
      wt[k] = weight[k];
    }
  }
  LC_ENTER(ctx);
  const size_t row_bytes = (size_t)n * W * sizeof(float);
  int rows = cfg->scratch_rows > 0 ? cfg->scratch_rows : (int)std::max<size_t>(1, kCoScratchBytes / row_bytes);
  rows = std::min(rows, H);
  const bool lds = n <= kCoLdsFrames;
  const int cthreads = lds ? kCoLdsThreads : kCoThreads;
  const size_t lds_bytes = lds ? (size_t)n * kCoLdsThreads * sizeof(float) : 0;
  const int tiles = (W + kCoThreads - 1) / kCoThreads;
  if ((uint64_t)n * rows * tiles >= ((uint64_t)1 << 31))
    LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_frames_coadd: n scratch_rows ceil(W / 256) must stay below 2^31");
  DeviceCall call(ctx);
  CoaddWarpArgs Wa;
  CoaddCombineArgs Ca;
  std::memset(&Wa, 0, sizeof(Wa));
  std::memset(&Ca, 0, sizeof(Ca));
  float *d_samples = nullptr, *d_image = nullptr, *d_wsum = nullptr;
  int32_t *d_count = nullptr, *d_rej = nullptr;
  LC_HIP(ctx, call.upload(frame, (size_t)n, &Wa.frame));
  LC_HIP(ctx, call.upload(affine, (size_t)n * 6, &Wa.affine));
  LC_HIP(ctx, call.upload((const float *)scale.data(), (size_t)n, &Wa.scale));
  LC_HIP(ctx, call.upload((const float *)wt.data(), (size_t)n, &Ca.weight));
  LC_HIP(ctx, call.alloc((size_t)n * rows * W, &d_samples));
  const size_t np = (size_t)H * W;
  LC_HIP(ctx, call.result(image, np, &d_image));
  LC_HIP(ctx, call.result(weight_out, np, &d_wsum));
  LC_HIP(ctx, call.result(count, np, &d_count));
  LC_HIP(ctx, call.result(n_rejected, np, &d_rej));
  Wa.n = n;
  Wa.W = W;
  Wa.h = f->h;
  Wa.w = f->w;
  Wa.order = cfg->order;
  Wa.x0 = x0;
  Wa.planes = f->planes;
  Wa.samples = d_samples;
  Ca.n = n;
  Ca.combine = cfg->combine;
  Ca.n_sigma = cfg->n_sigma;
  Ca.samples = d_samples;
  if (lds)
    LC_HIP(ctx, hipFuncSetAttribute((const void *)coadd_combine_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes));
  LC_HIP(ctx, call.start());
  for (int r0 = 0; r0 < H; r0 += rows) {
    const int rr = std::min(rows, H - r0);
    Wa.rows = rr;
    Wa.row0 = y0 + r0;
    hipLaunchKernelGGL(coadd_warp_kernel, dim3((unsigned)((size_t)n * rr * tiles)), dim3(kCoThreads), 0, ctx->stream, Wa);
    LC_HIP(ctx, hipGetLastError());
    const size_t snp = (size_t)rr * W, off = (size_t)r0 * W;
    Ca.np = Ca.stride = snp;
    Ca.image = d_image + off;
    Ca.wsum = d_wsum ? d_wsum + off : nullptr;
    Ca.count = d_count ? d_count + off : nullptr;
    Ca.nrej = d_rej ? d_rej + off : nullptr;
    const dim3 cgrid((unsigned)((snp + cthreads - 1) / cthreads));
    if (lds)
      hipLaunchKernelGGL(coadd_combine_kernel<true>, cgrid, dim3(cthreads), lds_bytes, ctx->stream, Ca);
    else
      hipLaunchKernelGGL(coadd_combine_kernel<false>, cgrid, dim3(cthreads), 0, ctx->stream, Ca);
    LC_HIP(ctx, hipGetLastError());
  }
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

}  // extern "C"
