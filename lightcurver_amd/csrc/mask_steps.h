// The stamp masks as launches on device pointers: what lc_ccdmask_stamps and lc_mask_cutouts (ccdmask.hip) run between
// their uploads and downloads, so that lc_frames_cut_stamps (cutout.hip) can run them on the stamps where it cut them.
// Every function enqueues on ctx->stream and returns without synchronising; the buffers belong to the caller.
#pragma once
#include "cosmics_device.h"
#include "device_call.h"
#include "lc_common.h"

namespace lc {

// stamp size and settings of a call: LC_OK, or the error code with ctx->err set ("<who>: ...")
int ccdmask_check(lc_ctx *ctx, const char *who, int n, const lc_ccdmask_cfg *cfg);

// one launch over K stamps; any output may be null
hipError_t ccdmask_launch(lc_ctx *ctx, int K, int n, const float *data, const lc_ccdmask_cfg *cfg, uint8_t *mask,
                          uint8_t *rowcol, uint8_t *bad_cols, uint8_t *bad_rows, float *sigma);

// y = x * x and a |= b over count elements (y may be x)
hipError_t square_launch(lc_ctx *ctx, const float *x, float *y, size_t count);
hipError_t or_launch(lc_ctx *ctx, uint8_t *a, const uint8_t *b, size_t count);

// The buffers of the whole of mask_cutout beside the stamps and the mask: mask_cutouts_scratch() allocates them from the
// call's pool for the switches that are on.
struct MaskCutoutsScratch {
  float *invar = nullptr;    // [K][n][n] the squared noise map (with do_cosmics)
  float *cosmics = nullptr;  // cosmics_scratch_bytes()
  uint8_t *lines = nullptr;  // [K][n][n] the rows and columns, when both switches are on
};
hipError_t mask_cutouts_scratch(DeviceCall &call, const lc_ctx *ctx, int K, int n, int do_bad_columns, int do_cosmics,
                                MaskCutoutsScratch *S);
// Every launch of lc_mask_cutouts with at least one switch on: data, noisemap [K][n][n] (noisemap read with do_cosmics;
// it may be S.invar, which lc_mask_cutouts uploads its noise map into), mask [K][n][n].  The arguments have been checked.
hipError_t mask_cutouts_launch(lc_ctx *ctx, int K, int n, const float *data, const float *noisemap, int do_bad_columns,
                               int do_cosmics, const lc_cosmics_cfg *cosmics_cfg, const lc_ccdmask_cfg *ccdmask_cfg,
                               const MaskCutoutsScratch &S, uint8_t *mask);

}  // namespace lc
