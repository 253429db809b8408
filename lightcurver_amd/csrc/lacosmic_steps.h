// The per-pixel steps of L.A.Cosmic that the stamp kernel (cosmics.hip) and the frame tiles (cosmics_frames.hip) share:
// the SPEC of DESIGN.md §5 "Cosmic-ray detection", every float32 operation in its order.  Device only.  They work on a
// square region of side R and row stride R whose pixel (ly, lx) is pixel (oy + ly, ox + lx) of a frame of h x w, for a
// workgroup of Threads lanes.  A tile is a region of R = 64 with a halo; a stamp is the region that is the whole frame,
// R = h = w = n at offset (0, 0).
#pragma once
#pragma clang fp contract(off)  // the SPEC fixes every rounding, whatever the including file sets

#include "lc_common.h"

namespace lc {

struct LaRegion {
  int oy, ox, h, w;
  __device__ __forceinline__ bool inside(int ly, int lx) const {
    const int gy = oy + ly, gx = ox + lx;
    return gy >= 0 && gy < h && gx >= 0 && gx < w;
  }
};

// step 0 at one pixel: counts, noise (0 without a variance) and mask from the value d, the inverse variance iv (read
// with have_var only) and the caller's input mask
__device__ __forceinline__ void la_input(float d, bool have_var, float iv, bool inmask, float gain, float gain2,
                                         float vhole, float *c_out, float *n_out, bool *m_out) {
  float c = gain * d;
  bool hole = !__builtin_isfinite(d);
  float v = 0.f;
  if (have_var) {
    hole = hole || !__builtin_isfinite(iv) || iv <= 0.f;
    v = iv * gain2;
  }
  if (hole) {
    c = 0.f;
    v = vhole;
  }
  *c_out = c;
  *n_out = have_var ? sqrtf(v) : 0.f;
  *m_out = hole || inmask;
}

template <int K>
__device__ __forceinline__ float la_median_net(float (&v)[K]) {
#pragma unroll
  for (int pass = 0; pass < K; ++pass) {
#pragma unroll
    for (int i = pass & 1; i + 1 < K; i += 2) {
      const float a = v[i], b = v[i + 1];
      v[i] = fminf(a, b);
      v[i + 1] = fmaxf(a, b);
    }
  }
  return v[K / 2];
}

// One pass of a separable median over the region: 1 x K along rows (stride 1) or K x 1 along columns (stride R).  The
// (K - 1) / 2 pixels at the FRAME's edge keep the input; so does a pixel whose window leaves the region: in a tile it
// lies in the halo, farther out than anything the tile's result reads.
template <int K, bool kRows, int Threads>
__device__ __forceinline__ void la_med_pass(const float *X, float *Y, int R, const LaRegion &T) {
  constexpr int hh = K / 2;
  const int np = R * R;
  for (int p = threadIdx.x; p < np; p += Threads) {
    const int ly = p / R, lx = p - ly * R;
    const int cl = kRows ? lx : ly;
    const int cf = (kRows ? T.ox : T.oy) + cl, nf = kRows ? T.w : T.h;
    float out = X[p];
    if (cf >= hh && cf < nf - hh && cl >= hh && cl < R - hh) {
      float v[K];
#pragma unroll
      for (int t = 0; t < K; ++t) v[t] = X[p + (t - hh) * (kRows ? 1 : R)];
      out = la_median_net<K>(v);
    }
    Y[p] = out;
  }
}

// Y = 1 x K median along rows, then K x 1 along columns (T1 is the row pass's output)
template <int K, int Threads>
__device__ __forceinline__ void la_sep_median(const float *X, float *T1, float *Y, int R, const LaRegion &T) {
  la_med_pass<K, true, Threads>(X, T1, R, T);
  __syncthreads();
  la_med_pass<K, false, Threads>(T1, Y, R, T);
  __syncthreads();
}

// 3 x 3 dilation, clipped at the region's edge (a tile keeps B at 0 outside the frame, which clips it there)
__device__ __forceinline__ bool la_dil3(const uint8_t *B, int ly, int lx, int R) {
  bool r = false;
  for (int y = max(ly - 1, 0); y <= min(ly + 1, R - 1); ++y)
    for (int x = max(lx - 1, 0); x <= min(lx + 1, R - 1); ++x) r |= B[y * R + x] != 0;
  return r;
}

__device__ __forceinline__ float la_clip0(float v) { return v < 0.f ? 0.f : v; }

// step 2a at region pixel (ly, lx): the four sub-pixels of its 2 x 2 block on the subsampled grid, the ring of that
// grid (the frame's) = 0
__device__ __forceinline__ float la_laplace(const float *C, int ly, int lx, int R, const LaRegion &T) {
  const int p = ly * R + lx, gy = T.oy + ly, gx = T.ox + lx;
  const float c = C[p], c4 = 4.0f * c;
  const bool top = gy <= 0, bottom = gy >= T.h - 1, left = gx <= 0, right = gx >= T.w - 1;
  // (at the region's edge, inside the frame, the neighbour is not held: such a pixel lies in the halo's outer ring)
  const float up = (top || ly == 0) ? 0.f : C[p - R], down = (bottom || ly == R - 1) ? 0.f : C[p + R];
  const float lf = (left || lx == 0) ? 0.f : C[p - 1], rt = (right || lx == R - 1) ? 0.f : C[p + 1];
  const float tl = (top || left) ? 0.f : la_clip0(c4 - (((up + c) + lf) + c));
  const float tr = (top || right) ? 0.f : la_clip0(c4 - (((up + c) + c) + rt));
  const float bl = (bottom || left) ? 0.f : la_clip0(c4 - (((c + down) + lf) + c));
  const float br = (bottom || right) ? 0.f : la_clip0(c4 - (((c + down) + c) + rt));
  return ((tl + tr) + (bl + br)) * 0.25f;
}

}  // namespace lc
