// Exact circular-aperture sums (DESIGN.md §5 "Aperture sums" is the SPEC).
//
// The reference takes the starting fluxes of the ROI's point sources from photutils.aperture_photometry(np.nanmedian(data,
// 0), CircularAperture(positions, r)) (lightcurver/processes/roi_modelling.py:198-204): the weight of a pixel is the area
// of its square inside the circle.  Here P apertures on K images are summed by ONE launch, on images that are uploaded
// with the call (lc_aperture_sums) or already live on the device (lc_frames_aperture_sums).
//
// The kernel: one wave64 per aperture, four apertures per workgroup.  The lanes run over a flat index of the circle's
// bounding box clipped to the image, so that an ROI-sized aperture (r = 3, box 8 x 8) fills the wave in one pass.  A pixel
// whose farthest corner lies inside the circle weighs 1 and one whose nearest point lies outside weighs 0; only the rim
// evaluates the closed form, in float64 (in float32 the four terms of size pi r^2 / 4 cancel to 1e-2 of a pixel at r = 20
// .. 64).  Each lane adds its pixels in index order, the wave reduces with a fixed butterfly and lane 0 stores: what an
// aperture gets depends on nothing but the aperture and its image, bit for bit.  No LDS, no atomics.
#include <cmath>
#include <cstring>

#include "device_call.h"
#include "frames_state.h"
#include "lc_common.h"
#include "noise_pixel.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kApertureThreads = 256;
constexpr int kAperturesPerGroup = kApertureThreads / kWave;

struct ApertureArgs {
  int h, w;
  unsigned P;
  const float *data;           // [K][h][w]
  const float *error;          // [K][h][w] nullable
  const uint8_t *mask;         // [K][h][w] nullable
  const float *exptime, *rms;  // [K], both or neither: the error is the noise of noise_pixel.h (error is null then)
  const int32_t *image;        // [P]
  const double *xy, *r;        // [P][2], [P]
  double *sum, *sum_err, *area, *bad_area;  // [P]; all but sum nullable
};

// the antiderivative of sqrt(r^2 - t^2), 0 <= t <= r
__device__ __forceinline__ double aperture_F(double t, double r, double r2) {
  const double s = sqrt((r - t) * (r + t));
  return 0.5 * (t * s + r2 * atan2(t, s));
}

// the signed area of the circle of radius r about the origin inside [0, x] x [0, y], odd in x and in y
__device__ __forceinline__ double aperture_Q(double x, double y, double r, double r2) {
  const double ax = fmin(fabs(x), r), ay = fmin(fabs(y), r);
  double q;
  if (ax * ax + ay * ay <= r2) {
    q = ax * ay;
  } else {
    const double xk = sqrt((r - ay) * (r + ay));
    q = xk * ay + aperture_F(ax, r, r2) - aperture_F(xk, r, r2);
  }
  return (x < 0.0) != (y < 0.0) ? -q : q;
}

// the area of the pixel [x0, x1] x [y0, y1] (relative to the centre) inside the circle, in [0, 1]
__device__ __forceinline__ double aperture_fraction(double x0, double x1, double y0, double y1, double r, double r2) {
  const double fx = fmax(fabs(x0), fabs(x1)), fy = fmax(fabs(y0), fabs(y1));
  if (fx * fx + fy * fy <= r2) return 1.0;
  const double nx = (x0 <= 0.0 && x1 >= 0.0) ? 0.0 : fmin(fabs(x0), fabs(x1));
  const double ny = (y0 <= 0.0 && y1 >= 0.0) ? 0.0 : fmin(fabs(y0), fabs(y1));
  if (nx * nx + ny * ny >= r2) return 0.0;
  const double f = aperture_Q(x1, y1, r, r2) - aperture_Q(x0, y1, r, r2) - aperture_Q(x1, y0, r, r2) + aperture_Q(x0, y0, r, r2);
  return fmin(fmax(f, 0.0), 1.0);
}

__global__ __launch_bounds__(kApertureThreads) void aperture_sums_kernel(ApertureArgs A) {
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned p = blockIdx.x * kAperturesPerGroup + (threadIdx.x >> 6);  // P + 3 < 2^32
  if (p >= A.P) return;  // the whole wave
  const int h = A.h, w = A.w, k = A.image[p];
  const double xc = A.xy[2 * (size_t)p], yc = A.xy[2 * (size_t)p + 1], r = A.r[p], r2 = r * r;
  // the pixels whose square reaches into (xc - r, xc + r) x (yc - r, yc + r), clipped to the image; compared as doubles
  // before they become ints: a centre may lie anywhere
  const double jlo = fmax(0.0, floor(xc - r + 0.5)), jhi = fmin((double)(w - 1), ceil(xc + r - 0.5));
  const double ilo = fmax(0.0, floor(yc - r + 0.5)), ihi = fmin((double)(h - 1), ceil(yc + r - 0.5));
  const bool any = jlo <= jhi && ilo <= ihi;
  const int j0 = any ? (int)jlo : 0, i0 = any ? (int)ilo : 0;
  const int bw = any ? (int)jhi - j0 + 1 : 0, bh = any ? (int)ihi - i0 + 1 : 0;
  const int n = bw * bh;  // <= h w < 2^31
  const size_t plane = (size_t)k * h * w;
  const bool noisy = A.exptime != nullptr;
  const float t = noisy ? A.exptime[k] : 1.0f;
  const float trms2 = noisy ? noise_trms2(t, A.rms[k]) : 0.f;
  double s = 0.0, v = 0.0, a = 0.0, b = 0.0;
  for (int q = lane; q < n; q += kWave) {
    const int di = q / bw, i = i0 + di, j = j0 + (q - di * bw);
    const double f = aperture_fraction(((double)j - 0.5) - xc, ((double)j + 0.5) - xc, ((double)i - 0.5) - yc,
                                       ((double)i + 0.5) - yc, r, r2);
    if (!(f > 0.0)) continue;
    const size_t at = plane + (size_t)i * w + j;
    if (A.mask && A.mask[at]) continue;
    const float d = A.data[at];
    const float e = A.error ? A.error[at] : noisy ? noise_from_rms(d, t, trms2) : 0.f;
    if (isfinite(d) && isfinite(e)) {
      s = fma(f, (double)d, s);
      v = fma(f, (double)e * (double)e, v);
      a += f;
    } else {
      b += f;
    }
  }
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
    s += __shfl_xor(s, m);
    v += __shfl_xor(v, m);
    a += __shfl_xor(a, m);
    b += __shfl_xor(b, m);
  }
  if (lane == 0) {
    A.sum[p] = s;
    if (A.sum_err) A.sum_err[p] = sqrt(v);
    if (A.area) A.area[p] = a;
    if (A.bad_area) A.bad_area[p] = b;
  }
}

// what both entry points check of the aperture list; nullptr if it is sound
static const char *aperture_list_error(int P, int K, const int32_t *image, const double *xy, const double *r) {
  for (int p = 0; p < P; ++p) {
    if (image[p] < 0 || image[p] >= K) return "an image index outside [0, K)";
    if (!std::isfinite(xy[2 * (size_t)p]) || !std::isfinite(xy[2 * (size_t)p + 1])) return "a coordinate that is not finite";
    if (!std::isfinite(r[p]) || !(r[p] > 0.0)) return "a radius that is not finite or not > 0";
  }
  return nullptr;
}

// uploads the list, registers the outputs, launches and waits; A holds the images and the error source
static int aperture_run(lc_ctx *ctx, ApertureArgs &A, DeviceCall &call, int P, const int32_t *image, const double *xy,
                        const double *r, double *sum, double *sum_err, double *area, double *bad_area, float *kernel_ms) {
  A.P = (unsigned)P;
  LC_HIP(ctx, call.upload(image, (size_t)P, &A.image));
  LC_HIP(ctx, call.upload(xy, 2 * (size_t)P, &A.xy));
  LC_HIP(ctx, call.upload(r, (size_t)P, &A.r));
  LC_HIP(ctx, call.result(sum, (size_t)P, &A.sum));
  LC_HIP(ctx, call.result(sum_err, (size_t)P, &A.sum_err));
  LC_HIP(ctx, call.result(area, (size_t)P, &A.area));
  LC_HIP(ctx, call.result(bad_area, (size_t)P, &A.bad_area));
  LC_HIP(ctx, call.start());
  const unsigned groups = ((unsigned)P + kAperturesPerGroup - 1) / kAperturesPerGroup;
  hipLaunchKernelGGL(aperture_sums_kernel, dim3(groups), dim3(kApertureThreads), 0, ctx->stream, A);
  LC_HIP(ctx, hipGetLastError());
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

}  // namespace lc

using namespace lc;

extern "C" {

int lc_aperture_sums(lc_ctx *ctx, int K, int h, int w, const float *data, const float *error, const uint8_t *mask, int P,
                     const int32_t *image, const double *xy, const double *r, double *sum, double *sum_err, double *area,
                     double *bad_area, float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  if (K < 1 || h < 1 || w < 1 || P < 1 || !data || !image || !xy || !r || !sum)
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_aperture_sums: invalid argument");
  if (sum_err && !error) LC_FAIL(ctx, LC_ERR_INVALID, "lc_aperture_sums: sum_err needs an error map");
  if ((int64_t)K * h * w >= ((int64_t)1 << 31)) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_aperture_sums: K h w must stay below 2^31");
  if (const char *why = aperture_list_error(P, K, image, xy, r)) LC_FAIL(ctx, LC_ERR_INVALID, std::string("lc_aperture_sums: ") + why);
  LC_ENTER(ctx);
  const size_t tot = (size_t)K * h * w;
  DeviceCall call(ctx);
  ApertureArgs A;
  std::memset(&A, 0, sizeof(A));
  A.h = h;
  A.w = w;
  LC_HIP(ctx, call.upload(data, tot, &A.data));
  LC_HIP(ctx, call.upload(error, tot, &A.error));
  LC_HIP(ctx, call.upload(mask, tot, &A.mask));
  return aperture_run(ctx, A, call, P, image, xy, r, sum, sum_err, area, bad_area, kernel_ms);
}

int lc_frames_aperture_sums(lc_frames *f, int P, const int32_t *frame, const double *xy, const double *r,
                            const float *exptime, const float *rms, int with_error, double *sum, double *sum_err,
                            double *area, double *bad_area, float *kernel_ms) {
  if (!f) return LC_ERR_INVALID;
  lc_ctx *ctx = f->ctx;
  const int K = f->K;
  if (P < 1 || !frame || !xy || !r || !sum) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_aperture_sums: invalid argument");
  if (sum_err && !with_error) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_aperture_sums: sum_err needs with_error");
  if (with_error && (!exptime || !rms) && !f->imported)
    LC_FAIL(ctx, LC_ERR_INVALID,
            "lc_frames_aperture_sums: with_error needs exptime and rms, or a frame set that has been imported");
  if (exptime)
    for (int k = 0; k < K; ++k)
      if (!std::isfinite(exptime[k]) || !(exptime[k] > 0.0f))
        LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_aperture_sums: an exposure time that is not finite or not > 0");
  if (const char *why = aperture_list_error(P, K, frame, xy, r))
    LC_FAIL(ctx, LC_ERR_INVALID, std::string("lc_frames_aperture_sums: ") + why);
  LC_ENTER(ctx);
  DeviceCall call(ctx);
  ApertureArgs A;
  std::memset(&A, 0, sizeof(A));
  A.h = f->h;
  A.w = f->w;
  A.data = f->planes;
  if (with_error) {
    A.exptime = f->exptime;
    A.rms = f->rms;
    if (exptime) LC_HIP(ctx, call.upload(exptime, (size_t)K, &A.exptime));
    if (rms) LC_HIP(ctx, call.upload(rms, (size_t)K, &A.rms));
  }
  return aperture_run(ctx, A, call, P, frame, xy, r, sum, sum_err, area, bad_area, kernel_ms);
}

}  // extern "C"
