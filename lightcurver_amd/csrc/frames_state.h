// The frame set that stays on the device (lc_frames of include/lcmi.h): what cutout.hip creates, imports and cuts
// stamps from, and what aperture.hip sums apertures on.
#pragma once
#include "device_call.h"
#include "lc_common.h"

struct lc_frames {
  lc_ctx *ctx = nullptr;
  int K = 0, h = 0, w = 0;
  bool imported = false;
  lc::DevPool pool;         // everything below
  float *planes = nullptr;  // [K][h][w]: the raw frames, sub after the import
  float *sub = nullptr;     // [K][h][w]: the import's output until it takes the place of planes
  float *exptime = nullptr, *rms = nullptr;  // [K]: recorded by the import
};
