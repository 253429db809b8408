// The noise of one pixel from the frame's background rms, as the reference forms it when it cuts a stamp
// (lightcurver/processes/cutout_making.py:43-51): in electrons, then back to electrons per second.  One definition for
// lc_prepare_stamps (prep.hip) and lc_frames_cut_stamps (cutout.hip), so that both give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace lc {

// d in electrons per second, t the exposure time, trms2 = (t rms)^2.  NaN data keeps the noise NaN, as in numpy.
__device__ __forceinline__ float noise_from_rms(float d, float t, float trms2) {
  const float e = d * t;
  const float s = fmaxf(sqrtf(trms2 + fabsf(e)), 1e-7f) / t;
  return e != e ? e : s;
}

// (t rms)^2 in the two roundings of the reference's float32 restatement
__device__ __forceinline__ float noise_trms2(float t, float rms) {
  const float trms = t * rms;
  return trms * trms;
}

}  // namespace lc
