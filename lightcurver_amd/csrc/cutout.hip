// A frame set that stays on the device, and the stamps cut from it (DESIGN.md §5 "Stamp cutting").
//
// The reference cuts one stamp at a time on the host (lightcurver/processes/cutout_making.py:23-51: Cutout2D(mode=
// 'partial', fill_value=nan) on the sky-subtracted frame, then the noise map from the frame's background rms).  Here the
// frames are uploaded once (lc_frames_create), imported where they lie (lc_frames_import: the launches of
// lc_import_frames, frame_steps.h) and every stamp of one size is cut by ONE launch (lc_frames_cut_stamps): the work is a
// few hundred kilobytes and bound by the launch, so neither a launch per stamp nor one per frame would do.  The masks of
// lc_mask_cutouts (mask_steps.h) then run on the stamps where the cut left them.
//
// The cut kernel: workgroup (s, c) takes chunk c of stamp s.  Consecutive lanes take consecutive pixels of a stamp row,
// which are consecutive in the frame: the loads coalesce although x0 is arbitrary (so they stay scalar); where n is a
// multiple of 4 a lane takes four pixels of a row and stores them as one float4.  Frame offsets are size_t: frame * h * w
// passes 2^31 for any real set.
#include <cmath>
#include <cstring>
#include <vector>

#include "device_call.h"
#include "frame_steps.h"
#include "frames_state.h"
#include "lc_common.h"
#include "mask_steps.h"
#include "noise_pixel.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kCutThreads = 256;
constexpr int kCutMaxChunks = 1024;  // chunks of a stamp in the grid; a larger stamp strides

struct CutArgs {
  int n, h, w;
  const float *planes;             // [K][h][w]
  const int32_t *frame, *y0, *x0;  // [S]
  const float *exptime, *rms;      // [K], both or neither (neither: no noise map)
  float *data, *noise;             // [S][n][n]; noise nullable
  int32_t *n_inside;               // [S] nullable
};

// V pixels of a row per lane (V = 4 needs n % 4 == 0: the four lie in one row and the store is aligned)
template <int V>
__global__ __launch_bounds__(kCutThreads) void cut_stamps_kernel(CutArgs A) {
  const int s = blockIdx.x, n = A.n, h = A.h, w = A.w;
  const int y0 = A.y0[s], x0 = A.x0[s], k = A.frame[s];
  const float *plane = A.planes + (size_t)k * h * w;
  const bool noisy = A.noise != nullptr;
  const float t = noisy ? A.exptime[k] : 1.0f;
  const float trms2 = noisy ? noise_trms2(t, A.rms[k]) : 0.f;
  const size_t base = (size_t)s * n * n;
  const int groups = n * n / V;  // S n n < 2^31
  for (int q = blockIdx.y * kCutThreads + threadIdx.x; q < groups; q += gridDim.y * kCutThreads) {
    const int p = q * V, i = p / n, j = p - i * n;
    const int yy = y0 + i;
    const bool row_in = yy >= 0 && yy < h;
    const float *row = plane + (size_t)(row_in ? yy : 0) * w;
    float d[V], e[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int xx = x0 + j + v;
      d[v] = (row_in && xx >= 0 && xx < w) ? row[xx] : __builtin_nanf("");
      e[v] = noisy ? noise_from_rms(d[v], t, trms2) : 0.f;
    }
    if constexpr (V == 4) {
      *reinterpret_cast<float4 *>(A.data + base + p) = make_float4(d[0], d[1], d[2], d[3]);
      if (noisy) *reinterpret_cast<float4 *>(A.noise + base + p) = make_float4(e[0], e[1], e[2], e[3]);
    } else {
      A.data[base + p] = d[0];
      if (noisy) A.noise[base + p] = e[0];
    }
  }
  if (A.n_inside && blockIdx.y == 0 && threadIdx.x == 0) {
    // the overlap is a rectangle; the host has checked that it is not empty
    const int ny = min(h, y0 + n) - max(0, y0), nx = min(w, x0 + n) - max(0, x0);
    A.n_inside[s] = ny * nx;
  }
}

static hipError_t cut_launch(lc_ctx *ctx, int S, const CutArgs &A) {
  const int V = A.n % 4 == 0 ? 4 : 1;
  const int groups = A.n * A.n / V;
  const dim3 grid((unsigned)S, (unsigned)std::min((groups + kCutThreads - 1) / kCutThreads, kCutMaxChunks));
  if (V == 4)
    hipLaunchKernelGGL(cut_stamps_kernel<4>, grid, dim3(kCutThreads), 0, ctx->stream, A);
  else
    hipLaunchKernelGGL(cut_stamps_kernel<1>, grid, dim3(kCutThreads), 0, ctx->stream, A);
  return hipGetLastError();
}

// the sizes of one cut: S n n < 2^31 (the stamps' flat index is an int in the mask kernels, and in the cut's loop)
static bool cut_fits(int64_t S, int64_t n) { return n >= 1 && S >= 1 && n <= 46340 && S * n * n < ((int64_t)1 << 31); }

}  // namespace lc

using namespace lc;

extern "C" {

int lc_frames_create(lc_ctx *ctx, int K, int h, int w, const float *data, lc_frames **out) {
  if (!ctx) return LC_ERR_INVALID;
  if (!out || !data || K < 1 || h < 1 || w < 1) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_create: invalid argument");
  if ((int64_t)h * w >= ((int64_t)1 << 31)) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_frames_create: frames of 2^31 pixels or more");
  LC_ENTER(ctx);
  lc_frames *f = new lc_frames();
  f->ctx = ctx;
  f->K = K;
  f->h = h;
  f->w = w;
  const size_t tot = (size_t)K * h * w;
  hipError_t e = f->pool.alloc(tot, &f->planes);
  if (e == hipSuccess) e = f->pool.alloc((size_t)K, &f->exptime);
  if (e == hipSuccess) e = f->pool.alloc((size_t)K, &f->rms);
  if (e == hipSuccess) e = hipMemcpyAsync(f->planes, data, tot * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the caller's buffer is free again on return
  if (e != hipSuccess) {
    delete f;
    LC_FAIL(ctx, LC_ERR_DEVICE, std::string("lc_frames_create: ") + hipGetErrorString(e));
  }
  *out = f;
  return LC_OK;
}

void lc_frames_destroy(lc_frames *f) {
  if (!f) return;
  (void)hipSetDevice(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  delete f;
}

int lc_frames_info(lc_frames *f, int *K, int *h, int *w, int *imported) {
  if (!f) return LC_ERR_INVALID;
  if (K) *K = f->K;
  if (h) *h = f->h;
  if (w) *w = f->w;
  if (imported) *imported = f->imported ? 1 : 0;
  return LC_OK;
}

int lc_frames_get(lc_frames *f, int first, int count, float *out) {
  if (!f) return LC_ERR_INVALID;
  lc_ctx *ctx = f->ctx;
  if (!out || first < 0 || count < 1 || (int64_t)first + count > f->K)
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_get: invalid argument");
  LC_ENTER(ctx);
  const size_t hw = (size_t)f->h * f->w;
  LC_HIP(ctx, hipMemcpyAsync(out, f->planes + (size_t)first * hw, (size_t)count * hw * sizeof(float),
                             hipMemcpyDeviceToHost, ctx->stream));
  LC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LC_OK;
}

}  // extern "C"

// lc_frames_import (dcfg not read) and lc_frames_import_deblended
static int frames_import(const char *who, bool deblended, lc_frames *f, const float *exptime, const lc_background_cfg *bcfg,
                         const lc_extract_cfg *ecfg, const lc_deblend_cfg *dcfg, int mask_sources_first,
                         const lc_extract_cfg *mcfg, int max_objects, float *sub, float *mesh_back, float *mesh_rms,
                         float *globalback, float *globalrms, int32_t *bg_status, lc_extract_object *objects, int32_t *nobj,
                         int32_t *segmap, int32_t *ex_status, float *kernel_ms) {
  if (!f) return LC_ERR_INVALID;
  lc_ctx *ctx = f->ctx;
  const int K = f->K, h = f->h, w = f->w;
  if (f->imported) LC_FAIL(ctx, LC_ERR_INVALID, std::string(who) + ": the frame set has been imported already");
  const bool pointers_ok = globalback && globalrms && objects && nobj && ex_status;
  if (int rc = import_check(ctx, who, pointers_ok, K, h, w, exptime, bcfg, ecfg, mask_sources_first, mcfg, max_objects))
    return rc;
  if (deblended) {
    int code = 0;
    if (const char *why = deblend_cfg_error(dcfg, &code)) LC_FAIL(ctx, code, std::string(who) + ": " + why);
  }
  LC_ENTER(ctx);
  const size_t hw = (size_t)h * w, tot = (size_t)K * hw, meshes = (size_t)K * background_meshes(h, w, bcfg->bw, bcfg->bh);
  const std::vector<double> pivots = background_pivots();
  if (!f->sub) LC_HIP(ctx, f->pool.alloc(tot, &f->sub));  // sub does not alias the frames: the two-pass sky reads them again
  DeviceCall call(ctx);
  ImportBuffers I;
  BackgroundBuffers &G = I.G;
  ExtractBuffers &B = I.B;
  G.data = f->planes;
  G.sub = f->sub;
  G.globalrms = f->rms;
  I.exptime = f->exptime;
  LC_HIP(ctx, hipMemcpyAsync(f->exptime, exptime, (size_t)K * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  LC_HIP(ctx, call.upload(pivots.data(), pivots.size(), &G.cfac));
  call.download(sub, tot, (const float *)f->sub);
  LC_HIP(ctx, mesh_back ? call.result(mesh_back, meshes, &G.mesh_back) : call.alloc(meshes, &G.mesh_back));
  LC_HIP(ctx, mesh_rms ? call.result(mesh_rms, meshes, &G.mesh_rms) : call.alloc(meshes, &G.mesh_rms));
  LC_HIP(ctx, call.result(globalback, (size_t)K, &G.globalback));
  call.download(globalrms, (size_t)K, (const float *)f->rms);
  LC_HIP(ctx, call.result(bg_status, (size_t)K, &G.status));
  LC_HIP(ctx, call.alloc(meshes, &G.raw_back));
  LC_HIP(ctx, call.alloc(meshes, &G.raw_rms));
  LC_HIP(ctx, call.alloc(meshes, &G.zy));
  LC_HIP(ctx, call.result(objects, (size_t)K * max_objects, &B.objects));
  LC_HIP(ctx, call.result(nobj, (size_t)K, &B.nobj));
  LC_HIP(ctx, call.result(segmap, tot, &B.segmap));
  LC_HIP(ctx, call.result(ex_status, (size_t)K, &B.status));
  LC_HIP(ctx, extract_scratch(call, K, h, w, max_objects, true, &B));
  LC_HIP(ctx, call.alloc(tot, &I.var));
  if (mask_sources_first) {
    LC_HIP(ctx, call.alloc(tot, &I.mask));
    LC_HIP(ctx, call.alloc((size_t)K, &I.v0));
    LC_HIP(ctx, call.alloc((size_t)K, &I.mstatus));
    LC_HIP(ctx, call.alloc((size_t)K, &I.mnobj));
  }
  I.dcfg = deblended ? dcfg : nullptr;
  I.call = &call;
  LC_HIP(ctx, call.start());
  LC_HIP(ctx, import_launch(ctx, K, h, w, bcfg, ecfg, mask_sources_first, mcfg, max_objects, I));
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  for (int k = 0; k < K; ++k)
    if (ex_status[k] == 1) return LC_OK;  // a table was too small: the set stays raw for the caller's second import
  f->pool.release(f->planes);
  f->planes = f->sub;
  f->sub = nullptr;
  f->imported = true;
  return LC_OK;
}

extern "C" {

int lc_frames_import(lc_frames *f, const float *exptime, const lc_background_cfg *bcfg, const lc_extract_cfg *ecfg,
                     int mask_sources_first, const lc_extract_cfg *mcfg, int max_objects, float *sub, float *mesh_back,
                     float *mesh_rms, float *globalback, float *globalrms, int32_t *bg_status, lc_extract_object *objects,
                     int32_t *nobj, int32_t *segmap, int32_t *ex_status, float *kernel_ms) {
  return frames_import("lc_frames_import", false, f, exptime, bcfg, ecfg, nullptr, mask_sources_first, mcfg, max_objects, sub,
                       mesh_back, mesh_rms, globalback, globalrms, bg_status, objects, nobj, segmap, ex_status, kernel_ms);
}

int lc_frames_import_deblended(lc_frames *f, const float *exptime, const lc_background_cfg *bcfg, const lc_extract_cfg *ecfg,
                               const lc_deblend_cfg *dcfg, int mask_sources_first, const lc_extract_cfg *mcfg,
                               int max_objects, float *sub, float *mesh_back, float *mesh_rms, float *globalback,
                               float *globalrms, int32_t *bg_status, lc_extract_object *objects, int32_t *nobj,
                               int32_t *segmap, int32_t *ex_status, float *kernel_ms) {
  return frames_import("lc_frames_import_deblended", true, f, exptime, bcfg, ecfg, dcfg, mask_sources_first, mcfg,
                       max_objects, sub, mesh_back, mesh_rms, globalback, globalrms, bg_status, objects, nobj, segmap,
                       ex_status, kernel_ms);
}

int lc_cutout_supported(int n, int with_masks) {
  if (with_masks) return lc_cosmics_supported(n) && lc_ccdmask_supported(n) ? 1 : 0;
  return cut_fits(1, n) ? 1 : 0;
}

int lc_frames_cut_stamps(lc_frames *f, int S, int n, const int32_t *frame, const int32_t *y0, const int32_t *x0,
                         const float *exptime, const float *rms, int do_bad_columns, int do_cosmics,
                         const lc_cosmics_cfg *cosmics_cfg, const lc_ccdmask_cfg *ccdmask_cfg, float *data_out,
                         float *noisemap_out, uint8_t *mask_out, int32_t *n_inside, float *kernel_ms) {
  if (!f) return LC_ERR_INVALID;
  lc_ctx *ctx = f->ctx;
  const int K = f->K, h = f->h, w = f->w;
  const bool masks = do_bad_columns || do_cosmics;
  if (S < 1 || n < 1 || !frame || !y0 || !x0 || !data_out || (masks && !mask_out) || (do_cosmics && !cosmics_cfg) ||
      (do_bad_columns && !ccdmask_cfg))
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_cut_stamps: invalid argument");
  const bool noisy = noisemap_out || masks;
  if (noisy && ((!exptime || !rms) && !f->imported))
    LC_FAIL(ctx, LC_ERR_INVALID,
            "lc_frames_cut_stamps: a noise map or a mask needs exptime and rms, or a frame set that has been imported");
  if (exptime)
    for (int k = 0; k < K; ++k)
      if (!std::isfinite(exptime[k]) || !(exptime[k] > 0.0f))
        LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_cut_stamps: an exposure time that is not finite or not > 0");
  for (int s = 0; s < S; ++s) {
    if (frame[s] < 0 || frame[s] >= K) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_cut_stamps: a frame index outside the set");
    if ((int64_t)x0[s] + n <= 0 || x0[s] >= w || (int64_t)y0[s] + n <= 0 || y0[s] >= h)
      LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_cut_stamps: a stamp without one pixel in the frame");
  }
  if (!cut_fits(S, n) || (int64_t)std::max(h, w) + n >= ((int64_t)1 << 31))  // y0 + i and x0 + j are ints in the kernel
    LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_frames_cut_stamps: S n n must stay below 2^31");
  if (do_cosmics)
    if (int rc = cosmics_check(ctx, "lc_frames_cut_stamps", n, cosmics_cfg)) return rc;
  if (do_bad_columns)
    if (int rc = ccdmask_check(ctx, "lc_frames_cut_stamps", n, ccdmask_cfg)) return rc;
  LC_ENTER(ctx);
  const size_t tot = (size_t)S * n * n;
  DeviceCall call(ctx);
  CutArgs A;
  std::memset(&A, 0, sizeof(A));
  A.n = n;
  A.h = h;
  A.w = w;
  A.planes = f->planes;
  LC_HIP(ctx, call.upload(frame, (size_t)S, &A.frame));
  LC_HIP(ctx, call.upload(y0, (size_t)S, &A.y0));
  LC_HIP(ctx, call.upload(x0, (size_t)S, &A.x0));
  if (noisy) {
    A.exptime = f->exptime;
    A.rms = f->rms;
    if (exptime) LC_HIP(ctx, call.upload(exptime, (size_t)K, &A.exptime));
    if (rms) LC_HIP(ctx, call.upload(rms, (size_t)K, &A.rms));
    // the masks read the noise map whether or not the caller takes it
    LC_HIP(ctx, noisemap_out ? call.result(noisemap_out, tot, &A.noise) : call.alloc(tot, &A.noise));
  }
  LC_HIP(ctx, call.result(data_out, tot, &A.data));
  LC_HIP(ctx, call.result(n_inside, (size_t)S, &A.n_inside));
  uint8_t *d_mask = nullptr;
  MaskCutoutsScratch M;
  if (masks) {
    LC_HIP(ctx, call.result(mask_out, tot, &d_mask));
    LC_HIP(ctx, mask_cutouts_scratch(call, ctx, S, n, do_bad_columns, do_cosmics, &M));
  } else if (mask_out) {
    std::memset(mask_out, 0, tot);
  }
  LC_HIP(ctx, call.start());
  LC_HIP(ctx, cut_launch(ctx, S, A));
  if (masks)
    LC_HIP(ctx, mask_cutouts_launch(ctx, S, n, A.data, A.noise, do_bad_columns, do_cosmics, cosmics_cfg, ccdmask_cfg, M, d_mask));
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

}  // extern "C"
