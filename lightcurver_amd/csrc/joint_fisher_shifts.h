// The dx_e, dy_e columns of lc_joint_fisher_shifts (the Fisher information with the epochs' translations free), gfx950.
//
// Column of dx_e: sqrt(w) (ss sum_i df/dX_i - ss (cos a_e B_x - sin a_e B_y)), of dy_e: sqrt(w) (ss sum_i df/dY_i -
// ss (sin a_e B_x + cos a_e B_y)).  The point-source part comes from joint_fisher_tmpl_kernel (shifts mode), one pair of
// values per source and pixel in a scratch that is added here in source order.  B_x = D_ss[s_e (*) H_x], B_y likewise: H_x,
// H_y are the derivatives of the resampled background with respect to the sample position, in the cell floor selects, clamped
// at the edge (bilinear_h of joint_kernels.h, restated for a run-time N).  Two kernels:
//   1. joint_fisher_shift_field_kernel: the zero-padded ss x ss sliding box sums A2[y][x] = sum_{s,t < ss} H[y + s][x + t] of
//      both fields, rows y = -(ss - 1) .. N - 1, columns x = c - N + 1 .. N - ss + c (everything a tap can touch: no bounds
//      in the convolution).  With xo = x - (c - N + 1) a row is stored as ss classes xo % ss of 2 n entries xo / ss, so that
//      the lanes of a wave (consecutive data columns V, x = ss V + c - q) read consecutive floats.
//   2. joint_fisher_shift_cols_kernel: B[U][V] = sum_{p,q} psf[p][q] A2[ss U + c - p][ss V + c - q] directly, n^2 N^2
//      multiply-adds per field and epoch.  One wave owns kFsRows data rows x 64 data columns and walks the rows y of A2: a
//      loaded pair (A2_x, A2_y) serves the kFsRows rows at once, each with its own PSF row p = ss U + c - y, whose entries
//      are wave-uniform (scalar loads; a row outside the PSF is replaced by a row of zeros).  float32, fixed order: q
//      ascending within a row of A2, the rows' sums added in ascending y.  Then the mix and the two columns of the slab.
// No atomics anywhere: two calls agree bit for bit.
// A batch of stars (lc_joint_groups_fisher_shifts): the field kernel reads the background of the epoch's own star
// (FisherShiftArgs::group); the column kernel never reads h itself, only the fields, and is the same for both.
#pragma once
#include <hip/hip_runtime.h>

#include "joint_fisher_positions.h"

namespace lc {

constexpr int kFsRows = 8;  // data rows per wave of the column kernel

struct FisherShiftArgs {
  const float *psf;   // [E][N][N]
  const float *wgt;   // [E][n][n]
  const float *h;     // [N][N], or null: no background pass
  const float *dx, *dy, *alpha;
  const float *gsh;   // [chunk][n n][2 M] (FisherTmplArgs::gsh)
  float *a2;          // [N] zeros, then [chunk][2][N + ss - 1][2 N]
  float *slab;        // [chunk][n n][32]
  int e0, M, n, ss, N, col;  // col: the column of dx_e (M + mean), dy_e follows
  // lc_joint_groups_fisher_shifts with a background per star: the star of every epoch [E], h is [G][N][N] and epoch e reads
  // h + group[e] N N.  Null: one background.  (A batch without a background passes h = null: its h is zero by construction,
  // every background term an exact zero and x - 0 exact, so the columns are those of an object holding h = 0.)
  const int *group = nullptr;
};

inline size_t fisher_shift_a2_floats(int chunk, int n, int ss) {
  const size_t N = (size_t)n * ss;
  return N + (size_t)chunk * 2 * (N + ss - 1) * 2 * N;
}

// (joint_fisher_shifts.hip) the field kernel (skipped without h) and the column kernel over `epochs` epochs, in stream order
void launch_fisher_shift_cols(const FisherShiftArgs &A, int epochs, hipStream_t q);

#ifdef LC_FISHER_SHIFTS_KERNELS

// sample_coords and the two derivative outputs of bilinear_h (joint_kernels.h) for a run-time N, operation for operation
__device__ __forceinline__ void fs_field(const float *h, int N, int u, int v, float c0, float ca, float sa, float sdx, float sdy,
                                         float &dHx, float &dHy) {
  const float qx = ((float)v - c0) - sdx;
  const float qy = ((float)u - c0) - sdy;
  const float Xs = c0 + (ca * qx + sa * qy);
  const float Ys = c0 + (ca * qy - sa * qx);
  const float x0f = floorf(Xs), y0f = floorf(Ys);
  const float fx = Xs - x0f, fy = Ys - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;
  const int xa = min(max(x0, 0), N - 1), xb = min(max(x0 + 1, 0), N - 1);
  const int ya = min(max(y0, 0), N - 1), yb = min(max(y0 + 1, 0), N - 1);
  const float h00 = h[ya * N + xa], h01 = h[ya * N + xb], h10 = h[yb * N + xa], h11 = h[yb * N + xb];
  const float top = h00 + fx * (h01 - h00), bot = h10 + fx * (h11 - h10);
  dHx = (1.f - fy) * (h01 - h00) + fy * (h11 - h10);
  dHy = bot - top;
}

// grid (blocks over the (N + ss - 1) x 2 N entries of one field, epochs of the chunk)
__global__ __launch_bounds__(kFpThreads) void joint_fisher_shift_field_kernel(FisherShiftArgs A) {
  const int b = blockIdx.y, e = A.e0 + b, N = A.N, ss = A.ss, NR = N + ss - 1, W = 2 * N, PWC = 2 * A.n;
  const int k = blockIdx.x * kFpThreads + threadIdx.x;
  if (k >= NR * W) return;
  const int yr = k / W, xo = k % W;
  const int c = (N - 1) / 2, y = yr - (ss - 1), x = xo + c - N + 1;
  const float c0 = (N - 1) * 0.5f;
  const float al = A.alpha[e] * 0.017453292519943295f;
  const float ca = cosf(al), sa = sinf(al);
  const float sdx = ss * A.dx[e], sdy = ss * A.dy[e];
  float sx = 0.f, sy = 0.f;
  for (int s = 0; s < ss; ++s)
    for (int t = 0; t < ss; ++t) {
      const int u = y + s, v = x + t;
      if (u < 0 || u >= N || v < 0 || v >= N) continue;
      float hx, hy;
      fs_field(A.h + (A.group ? (size_t)A.group[e] * N * N : 0), N, u, v, c0, ca, sa, sdx, sdy, hx, hy);  // its star's h
      sx += hx;
      sy += hy;
    }
  float *out = A.a2 + N + (size_t)b * 2 * NR * W + (size_t)yr * W + (xo % ss) * PWC + xo / ss;
  out[0] = sx;
  out[(size_t)NR * W] = sy;
}

// grid (ceil(waves / 4), epochs of the chunk); waves = ceil(n / kFsRows) ceil(n / 64), four to a workgroup
template <int SS>
__global__ __launch_bounds__(kFpThreads) void joint_fisher_shift_cols_kernel(FisherShiftArgs A) {
  const int b = blockIdx.y, e = A.e0 + b, n = A.n, N = A.N, M = A.M, nn = n * n;
  const int CC = (n + 63) / 64, RG = (n + kFsRows - 1) / kFsRows;
  const int item = blockIdx.x * (kFpThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= RG * CC) return;
  const int U0 = (item / CC) * kFsRows, V = (item % CC) * 64 + (threadIdx.x & 63);
  float accx[kFsRows], accy[kFsRows];
#pragma unroll
  for (int r = 0; r < kFsRows; ++r) accx[r] = accy[r] = 0.f;
  if (A.h) {
    const int NR = N + SS - 1, W = 2 * N, PWC = 2 * n, c = (N - 1) / 2;
    const float *zero = A.a2, *psf = A.psf + (size_t)e * N * N;
    // (a lane beyond the stamp reads what its last column reads and stores nothing)
    const float *fx = A.a2 + N + (size_t)b * 2 * NR * W + min(V, n - 1), *fy = fx + (size_t)NR * W;
    const int Ul = min(n, U0 + kFsRows) - 1;
    const int ylo = max(-(SS - 1), SS * U0 + c - (N - 1)), yhi = min(N - 1, SS * Ul + c);
    for (int y = ylo; y <= yhi; ++y) {
      const float *kr[kFsRows];
#pragma unroll
      for (int r = 0; r < kFsRows; ++r) {
        const int p = SS * (U0 + r) + c - y;
        kr[r] = (p >= 0 && p < N) ? psf + (size_t)p * N : zero;
      }
      const float *ax = fx + (size_t)(y + SS - 1) * W, *ay = fy + (size_t)(y + SS - 1) * W;
      float rx[kFsRows], ry[kFsRows];
#pragma unroll
      for (int r = 0; r < kFsRows; ++r) rx[r] = ry[r] = 0.f;
#pragma unroll 4
      for (int q = 0; q < N; ++q) {
        const unsigned t = N - 1 - q, off = (t % SS) * PWC + t / SS;
        const float a0 = ax[off], a1 = ay[off];
#pragma unroll
        for (int r = 0; r < kFsRows; ++r) {
          const float k = kr[r][q];
          rx[r] = fmaf(k, a0, rx[r]);
          ry[r] = fmaf(k, a1, ry[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < kFsRows; ++r) {
        accx[r] += rx[r];
        accy[r] += ry[r];
      }
    }
  }
  if (V >= n) return;
  const float al = A.alpha[e] * 0.017453292519943295f;
  const float ca = cosf(al), sa = sinf(al), fs = (float)SS;
  const float *w = A.wgt + (size_t)e * nn;
#pragma unroll
  for (int r = 0; r < kFsRows; ++r) {
    const int U = U0 + r;
    if (U >= n) break;
    const int px = U * n + V;
    const float *g = A.gsh + ((size_t)b * nn + px) * (2 * M);
    float sx = 0.f, sy = 0.f;
    for (int i = 0; i < M; ++i) {  // the sources in their order
      sx += g[2 * i];
      sy += g[2 * i + 1];
    }
    const float sw = sqrtf(w[px]);
    float *row = A.slab + ((size_t)b * nn + px) * kFpCols + A.col;
    row[0] = sw * (sx - fs * (ca * accx[r] - sa * accy[r]));
    row[1] = sw * (sy - fs * (sa * accx[r] + ca * accy[r]));
  }
}

#endif  // LC_FISHER_SHIFTS_KERNELS

}  // namespace lc
