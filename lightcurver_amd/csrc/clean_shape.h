// The float64 shape that sep's clean compares, and the wing of a brighter neighbour at an object's centre: item 5 (a) of
// the SPEC of DESIGN.md §5 "De-blending and cleaning of frame objects", which is that of "Source masking".  Device only.
// Which pairs are compared, and in which order, is the caller's: segment_kernel goes faint-first and skips merged
// objects, db_target_kernel takes every object on its own.
#pragma once
#pragma clang fp contract(off)  // the SPEC fixes every rounding, whatever the including file sets

#include <cmath>

#include "lc_common.h"

namespace lc {

struct CleanShape {
  double x, y, a, cxx, cyy, cxy, unit, amp, mth;
  long long s0;
  int npix, valid;
};

// The shape of an object from the sums of q, q x, q y, q x^2, q y^2, q x y over its pixels, q = snr * fix rounded to an
// integer and x, y counted from (x0, y0), each sum converted to double by the caller (they are non-negative, so a
// signed and an unsigned 64-bit sum give the same double).  t > 0 is an integer below 2^53 (at most 2^18 pixels of
// q < 2^26, or 2^12 of q <= 2^36), so s0 is the caller's sum exactly.  kth_bits: the bits of the minarea-th largest snr
// (used where the object has that many pixels).
__device__ __forceinline__ CleanShape clean_shape(double t, double sx, double sy, double sxx, double syy, double sxy,
                                                  double fix, int npix, int minarea, unsigned kth_bits, float thresh,
                                                  double x0, double y0) {
  const double twelfth = 1.0 / 12.0;
  const double mx = sx / t, my = sy / t;
  const double x2 = fmax(sxx / t - mx * mx, twelfth), y2 = fmax(syy / t - my * my, twelfth);
  double xy = sxy / t - mx * my;
  double det = x2 * y2 - xy * xy;
  if (det < 1.0 / 144.0) {
    xy = 0.0;
    det = x2 * y2;
  }
  const double half = 0.5 * (x2 + y2), dif = x2 - y2;
  const double root = sqrt(fmax(0.25 * (dif * dif) + xy * xy, 0.0));
  const double a = sqrt(half + root), b = sqrt(fmax(half - root, twelfth));
  CleanShape z;
  z.x = x0 + mx;
  z.y = y0 + my;
  z.a = a;
  z.cxx = y2 / det;
  z.cyy = x2 / det;
  z.cxy = -2.0 * xy / det;
  z.unit = M_PI * a * b;
  z.amp = (t * (1.0 / fix)) / (2.0 * z.unit);
  z.mth = npix >= minarea ? fmax((double)__uint_as_float(kth_bits) - (double)thresh, 0.0) : 0.0;
  z.s0 = (long long)t;
  z.npix = npix;
  z.valid = 1;
  return z;
}

// what the profile of `other` adds at the centre of `me`; 0 where it is too far, too faint or out of range
__device__ __forceinline__ double clean_wing(const CleanShape &me, const CleanShape &other, double thresh) {
  const double dx = me.x - other.x, dy = me.y - other.y;
  const double zone = 10.0 * (me.a + other.a);
  if (dx * dx + dy * dy >= zone * zone) return 0.0;
  const double ratio = other.amp / thresh;
  if (ratio <= 1.0) return 0.0;
  const double alpha = (ratio - 1.0) * other.unit / (double)other.npix;
  const double val = 1.0 + alpha * (other.cxx * dx * dx + other.cyy * dy * dy + other.cxy * dx * dy);
  return (1.0 < val && val < 1e10) ? other.amp / val : 0.0;
}

}  // namespace lc
