// The resampler of the co-add SPEC (DESIGN.md §5 "Co-addition of frames"), shared by coadd.hip and diffim.hip: one sample
// of a resident plane at a reference pixel.  Coordinates, floor and the all-taps-inside test in double; weights and the
// tap sum in float32, y-major.  NaN where a tap falls outside the frame.
#pragma once
#pragma clang fp contract(off)  // the SPEC fixes every rounding

#include "lc_common.h"

namespace lc {

// Keys' cubic convolution with a = -1/2 at offset t in [0, 1): the weights of the taps f - 1 .. f + 2
__device__ __forceinline__ void co_cubic(float t, float w[4]) {
  w[0] = ((2.0f - t) * t - 1.0f) * t / 2.0f;
  w[1] = ((3.0f * t - 5.0f) * t * t + 2.0f) / 2.0f;
  w[2] = ((4.0f - 3.0f * t) * t + 1.0f) * t / 2.0f;
  w[3] = (t - 1.0f) * t * t / 2.0f;
}

template <int TAPS>
__device__ __forceinline__ float co_sample(const float *img, int w, int ty, int tx, const float *wy, const float *wx) {
  float v = 0.0f;
#pragma unroll
  for (int a = 0; a < TAPS; ++a) {
    const float *row = img + (size_t)(ty + a) * w + tx;
#pragma unroll
    for (int b = 0; b < TAPS; ++b) {
      float t = row[b];
      t = t * wy[a];
      t = t * wx[b];
      v = v + t;
    }
  }
  return v;
}

// the sample of the h x w plane img at the reference pixel (x, y) under the affine M (reference -> frame), times scale
__device__ __forceinline__ float co_resample(const float *img, int h, int w, const double *M, double x, double y, int order,
                                             float scale) {
  const double xs = (M[0] * x + M[1] * y) + M[2], ys = (M[3] * x + M[4] * y) + M[5];
  const double fx = floor(xs), fy = floor(ys);
  const float tx = (float)(xs - fx), ty = (float)(ys - fy);
  const int before = order == 3 ? 1 : 0, after = order == 3 ? 2 : 1;
  float v = __builtin_nanf("");
  // (a coordinate that is not finite fails every comparison)
  if (fx >= (double)before && fx <= (double)(w - 1 - after) && fy >= (double)before && fy <= (double)(h - 1 - after)) {
    const int ix = (int)fx - before, iy = (int)fy - before;
    if (order == 3) {
      float wy[4], wx[4];
      co_cubic(ty, wy);
      co_cubic(tx, wx);
      v = co_sample<4>(img, w, iy, ix, wy, wx);
    } else {
      const float wy[2] = {1.0f - ty, ty}, wx[2] = {1.0f - tx, tx};
      v = co_sample<2>(img, w, iy, ix, wy, wx);
    }
    v = v * scale;
  }
  return v;
}

}  // namespace lc
