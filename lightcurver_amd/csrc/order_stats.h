// Order statistics on the order-preserving integer key of a float32, and the per-pixel robust combine of the SPECs of
// DESIGN.md §5 "Align and stack" and "Co-addition of frames", which is one algorithm.  Device only.  Where a sample
// and its weight come from, and which results are stored, is the caller's.
#pragma once
#pragma clang fp contract(off)  // the SPEC fixes every rounding, whatever the including file sets

#include "lc_common.h"

namespace lc {

// order-preserving image of a float in the unsigned integers, and back (exact both ways)
__device__ __forceinline__ unsigned float_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

constexpr unsigned kMissingKey = 0xFFFFFFFFu;  // the key of a NaN pattern: of no finite float, and never < a candidate
__device__ __forceinline__ unsigned float_key_or_missing(float x) {
  return __builtin_isfinite(x) ? float_key(x) : kMissingKey;
}

// The keys of ranks (m - 1) / 2 and m / 2 among the m > 0 keys of key(0 .. n) that are not kMissingKey: bitwise
// bisection, 32 counting passes over the samples, both middle elements at once.
template <class Key>
__device__ __forceinline__ void middle_keys(int n, int m, const Key &key, unsigned *lo, unsigned *hi) {
  const int klo = (m - 1) / 2, khi = m / 2;
  unsigned tlo = 0u, thi = 0u;
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned clo = tlo | (1u << bit), chi = thi | (1u << bit);
    int nlo = 0, nhi = 0;
    for (int k = 0; k < n; ++k) {
      const unsigned x = key(k);
      nlo += x < clo;
      nhi += x < chi;
    }
    if (nlo <= klo) tlo = clo;
    if (nhi <= khi) thi = chi;
  }
  *lo = tlo;
  *hi = thi;
}

struct Combined {
  int m, kept, rej;  // finite samples; of those, the ones in the weighted sums and the ones clipped
  float median;      // NaN where m == 0 or the median is not asked for
  float sw, swv;     // sum of w, sum of w x over the kept samples: 0 where m == 0
};

// The combine of the n samples key(0 .. n) with the weights weight(k), every sum sequential in the order of k:
// count and sum of the finite samples, the median (mean of the two middle elements), with `clip` the deviation about
// the mean and the rejection of the samples farther than n_sigma dev from the median, the weighted sums of the rest.
// `clip` needs `want_median`.  `median_only` leaves after the median.
template <class Key, class Weight>
__device__ __forceinline__ Combined robust_combine(int n, const Key &key, const Weight &weight, bool want_median,
                                                   bool clip, float n_sigma, bool median_only) {
  Combined c = {0, 0, 0, __builtin_nanf(""), 0.0f, 0.0f};
  float s = 0.0f;
  for (int k = 0; k < n; ++k) {
    const unsigned x = key(k);
    if (x != kMissingKey) {
      ++c.m;
      s = s + float_unkey(x);
    }
  }
  if (c.m == 0) return c;
  if (want_median) {
    unsigned tlo, thi;
    middle_keys(n, c.m, key, &tlo, &thi);
    const float lo = float_unkey(tlo), hi = float_unkey(thi);
    c.median = (c.m & 1) ? lo : 0.5f * (lo + hi);  // odd m: the two ranks are one
  }
  if (median_only) return c;
  bool all = true;
  float thr = 0.0f;
  if (clip) {
    const float mean = s / (float)c.m;
    float q = 0.0f;
    for (int k = 0; k < n; ++k) {
      const unsigned x = key(k);
      if (x != kMissingKey) {
        const float d = float_unkey(x) - mean;
        q = q + d * d;
      }
    }
    const float dev = sqrtf(q / (float)c.m);
    thr = n_sigma * dev;
    all = !__builtin_isfinite(dev);
  }
  for (int k = 0; k < n; ++k) {
    const unsigned x = key(k);
    if (x == kMissingKey) continue;
    const float v = float_unkey(x);
    if (all || fabsf(v - c.median) <= thr) {
      const float w = weight(k);
      c.sw = c.sw + w;
      c.swv = c.swv + w * v;
      ++c.kept;
    } else {
      ++c.rej;
    }
  }
  return c;
}

}  // namespace lc
