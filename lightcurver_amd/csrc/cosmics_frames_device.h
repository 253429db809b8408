// The frame form of the cosmic-ray kernels with device pointers (cosmics_frames.hip): what lc_detect_cosmics_frames runs
// between its copies, and what lc_frames_detect_cosmics runs on the resident planes of a frame set.
#pragma once
#include "device_call.h"
#include "lc_common.h"

namespace lc {

// frame shape, settings and chunking of a call: LC_OK, or the error code with ctx->err set ("<who>: ...")
int cosmics_frames_check(lc_ctx *ctx, const char *who, int h, int w, const lc_cosmics_cfg *cfg, int scratch_frames);

// the planes of one chunk of frames between the launches, and the per-frame control words
struct CosmicsFramesScratch {
  int chunk = 0;          // frames per chunk
  float *C = nullptr;     // [chunk][h][w] counts, cleaned in place
  float *N = nullptr;     // [chunk][h][w] noise, with a variance only
  uint8_t *M = nullptr;   // [chunk][h][w] mask
  uint8_t *CR = nullptr;  // [chunk][h][w] cosmics (2: waiting for the frame's fall-back value)
  int32_t *state = nullptr;
  uint32_t *hist = nullptr;
  int32_t *running = nullptr;
};

// frames per chunk: scratch_frames, or as many as a budget of 128 MiB holds (at least one), at most K
int cosmics_frames_chunk(int K, int h, int w, bool with_variance, int scratch_frames);
hipError_t cosmics_frames_scratch(DeviceCall &call, int K, int h, int w, bool with_variance, int scratch_frames,
                                  CosmicsFramesScratch *S);

// Device pointers of one call over K slots.  The data of slot k is plane frame[k] of `data` (plane k when frame is null).
// The variance is invar [K][h][w] (by slot), or, with exptime and rms (by PLANE), the square of the noise map
// lc::noise_from_rms gives, or neither (the SPEC's noise model).  inmask by slot.  Outputs by slot, each nullable.
// apply != 0 writes the flagged pixels of the slot's plane into `planes` (LC_COSMICS_SET_NAN / LC_COSMICS_SET_CLEAN).
struct CosmicsFramesIO {
  const float *data = nullptr;
  const int32_t *frame = nullptr;
  const float *invar = nullptr, *exptime = nullptr, *rms = nullptr;
  const uint8_t *inmask = nullptr;
  uint8_t *crmask = nullptr;
  float *clean = nullptr;
  int32_t *iters = nullptr, *n_flagged = nullptr;
  float *planes = nullptr;
  int apply = 0;
};

// every launch of the call on ctx->stream, chunk by chunk; reads one word back per iteration and chunk (the number of
// frames still running), so it synchronises the stream
hipError_t cosmics_frames_launch(lc_ctx *ctx, int K, int h, int w, const CosmicsFramesIO &io, const lc_cosmics_cfg *cfg,
                                 const CosmicsFramesScratch &S);

}  // namespace lc
