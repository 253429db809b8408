// Fisher information of the joint fit with the source positions free (lc_joint_fisher_positions), gfx950.
//
// Free parameters: a [E M], c_x [M], c_y [M] and optionally mean [E]; dx, dy, alpha and h stay at their current values, so the
// result is conditional on the registration and the background.  F = J^T diag(w) J (Gauss-Newton: independent of the data).
// Three steps:
//   1. joint_fisher_tmpl_kernel: the weighted columns sqrt(w) df/dtheta of one epoch as a pixel-major slab [b][n n][32].  The
//      scene of one source is rank one (gy x gx), so s (*) G is two 1-D passes over the PSF - no FFT, no h: a row pass with gx
//      and with dgx = gx (v - X) / sigma^2, then three column passes (gy R_g -> T, gy R_d -> dX, dgy R_g -> dY).  The ss x ss
//      block sum is folded into the tables (gxs[t] = sum_s gx[t + s]).  Table entries below 1e-30 of the table's peak are
//      skipped (beyond 10 high-resolution pixels of the source), which bounds both passes to 21 + ss - 1 taps.  The PSF rows
//      are streamed: one workgroup owns kFpBand data rows and forms the row pass of the PSF rows those need, nothing more.
//   2. joint_fisher_gram_kernel: F_e = T^T T over the 32 padded columns on the matrix cores.  v_mfma_f32_32x32x2_f32 with
//      the same register as both operands: lane l holds column l & 31 of pixel 2 step + (l >> 5), which is A[i][k] of
//      A = T^T and B[k][j] of B = T at once.  Four accumulators per wave over interleaved pixel streams (the dependent
//      accumulation has the latency of the instruction), each flushed into float64 after at most 128 pixels; the four waves'
//      float64 partials are added in a fixed order.  No atomics: two calls agree bit for bit.
//   3. joint_fisher_arrow_*: the arrowhead solve in float64.  Per epoch the Cholesky factor of the local block (a_e, mean_e),
//      B_e = F_loc^-1 F_x and F_x^T B_e; one workgroup adds the epochs in epoch order, S = F_cc - sum_e F_x^T B_e,
//      C_cc = S^-1; per epoch again C_x = -B_e C_cc and C_loc = F_loc^-1 + B_e C_cc B_e^T.
// Degenerate cases (the rules of joint_fisher_cov_kernel, continued): a parameter with a zero diagonal (the prior included
// for c) is left out, sigma = +inf and zero rows / columns of C; a Cholesky pivot of any local block or of S that is not
// above kFpPivot times its diagonal entry makes every C and sigma output NaN (F stays as computed).
//
// lc_joint_fisher_shifts (dx_e, dy_e free as well) runs the same three steps in their shifts mode: the local block is (a_e,
// mean_e, dx_e, dy_e), the template kernel also leaves every source's ss a dT/dX, ss a dT/dY for the two new columns, which
// joint_fisher_shifts.h writes before the Gram kernel, and the solve kernels are instantiated at the local capacity 11 beside 9.
// With shifts = 0 nothing of the existing call changes: same columns, values and bits.
//
// lc_joint_groups_fisher_shifts (a batch of stars, every star with its own positions and background) is the shifts mode with the
// positions fixed and the epoch -> star map `group`: the template kernel reads the positions of the epoch's star, the shift
// kernels its background, and the NaN rule holds per star - one verdict per star over that star's epochs (gstart), read by
// the back-substitution of each of its epochs.  group[e] is read where it is used: the arithmetic of an epoch is that of the
// one-object call, operation for operation.
//
// joint_fit.hip includes this file for the argument structures and the launchers; the kernels themselves are compiled by
// joint_fisher_positions.hip (LC_FISHER_POSITIONS_KERNELS), a translation unit of their own: the set of kernels of
// joint_fit.hip and their registers are pinned by tests/test_psf_budget_isa_cpu.py.
#pragma once
#include <hip/hip_runtime.h>

#include "lc_common.h"

namespace lc {

constexpr int kFpMaxSources = 8;     // = kMaxSources (joint_kernels.h)
constexpr double kFpPivot = 1e-6;    // = kFisherPivot (joint_fisher.h)

constexpr int kFpCols = 32;      // columns of the slab: a (M), mean (0 / 1), [dx, dy,] c_x (M), c_y (M), zero padding
constexpr int kFpThreads = 256;
constexpr int kFpBand = 16;      // data rows per workgroup of the template kernel
constexpr int kFpSpan = 24;      // table entries kept per source and axis at most (the 1e-30 cut leaves 21)
constexpr int kFpLocal = kFpMaxSources + 1, kFpShared = 2 * kFpMaxSources;
constexpr int kFpLocalShifts = kFpLocal + 2;  // lc_joint_fisher_shifts: a_e, mean_e, dx_e, dy_e
constexpr float kFpCut = 1e-30f;

struct FisherTmplArgs {
  const float *psf;  // [E][N][N]
  const float *wgt;  // [E][n][n]
  const float *a, *cx, *cy, *dx, *dy, *alpha;
  float *slab;       // [chunk][n n][32]
  int e0, M, n, ss, N, positions, mean;
  // lc_joint_fisher_shifts: the local block is (a, mean, dx, dy) - two more columns ahead of c_x, c_y, written by
  // joint_fisher_shift_cols_kernel (joint_fisher_shifts.h) - and every source leaves a ss dT/dX, a ss dT/dY of the scene
  // frame, neither rotated nor weighted, in gsh [chunk][n n][2 M] for that kernel to add in source order
  int shifts = 0;
  float *gsh = nullptr;
  // lc_joint_groups_fisher_shifts (batched star photometry): the star of every epoch [E]; source i of epoch e then sits at
  // cx, cy [group[e] M + i].  Null: one object, one set of positions
  const int *group = nullptr;
};

inline size_t fisher_tmpl_lds(int n, int ss) {
  const int N = n * ss;
  return (size_t)(4 * (N + ss) + 2 * (ss * kFpBand + kFpSpan) * n) * sizeof(float);
}

struct FisherGramArgs {
  const float *slab;  // [b][nn][32]
  int nn;
  double *Fd;         // [b][32][32]
};

struct FisherArrowArgs {
  const double *Fd;    // [E][32][32]
  double *Binv;        // [E][KL][KL]  F_loc^-1, zero rows / columns of the parameters left out (KL = 9, with the shifts 11)
  double *B;           // [E][KL][16]  F_loc^-1 F_x
  double *G;           // [E][16][16]  F_x^T B
  double *Ccc;         // [16][16]
  int *ok;             // [E + 1]: every epoch's factorisation, then the whole solve
  const float *prior;  // [4][M] (means and sigmas of c_x, c_y) or null
  int E, M, Lp, Sh;    // Sh = 2 M, or 0 with the positions fixed
  float *F_local, *F_cross, *F_shared, *C_local, *C_cross, *C_shared, *sigma_a, *sigma_mean, *sigma_c;
  int shifts = 0;      // the last two local parameters are dx_e, dy_e (local capacity kFpLocalShifts)
  float *sigma_dx = nullptr, *sigma_dy = nullptr;
  // lc_joint_groups_fisher_shifts: `stars` stars, star g owns the epochs [gstart[g], gstart[g + 1]), group [E] is the star of every
  // epoch.  The positions are fixed there (Sh = 0), and ok holds one verdict per star, [E + stars].  Null: one verdict for all
  const int *group = nullptr, *gstart = nullptr;
  int stars = 0;
};

// (joint_fisher_positions.hip) the template kernel on grid (bands, max(M, 1), epochs) with `lds` bytes; the Gram kernel on
// `epochs` workgroups; the three solve kernels over all E epochs, in stream order
void launch_fisher_tmpl(const FisherTmplArgs &A, int bands, int sources, int epochs, size_t lds, hipStream_t q);
void launch_fisher_gram(const FisherGramArgs &A, int epochs, hipStream_t q);
void launch_fisher_arrow(const FisherArrowArgs &A, hipStream_t q);

#ifdef LC_FISHER_POSITIONS_KERNELS

// grid (bands, max(M, 1), epochs of the chunk)
__global__ __launch_bounds__(kFpThreads) void joint_fisher_tmpl_kernel(FisherTmplArgs A) {
  extern __shared__ float fp_lds[];
  __shared__ int WIN[4];      // lo_x, hi_x, lo_y, hi_y: the table entries kept
  __shared__ double XY[4];    // X, Y, cos, sin
  const int tid = threadIdx.x, band = blockIdx.x, i = blockIdx.y, b = blockIdx.z, e = A.e0 + b;
  const int n = A.n, ss = A.ss, N = A.N, M = A.M, nn = n * n;
  const int Lp = M + (A.mean ? 1 : 0) + (A.shifts ? 2 : 0), P = Lp + (A.positions ? 2 * M : 0);
  const int U0 = band * kFpBand, U1 = min(n, U0 + kFpBand);
  const int TL = N + ss;  // table stride (N + ss - 1 entries used)
  float *GXS = fp_lds, *DGXS = GXS + TL, *GYS = DGXS + TL, *DGYS = GYS + TL;
  float *RG = DGYS + TL, *RD = RG + (ss * kFpBand + kFpSpan) * n;
  float *slab = A.slab + (size_t)b * nn * kFpCols;
  const float *w = A.wgt + (size_t)e * nn;

  if (i == 0) {  // the mean column and the padding (the column layout changes with the flags: nothing is left over)
    for (int idx = tid; idx < (U1 - U0) * n; idx += kFpThreads) {
      float *row = slab + (size_t)(U0 * n + idx) * kFpCols;
      if (A.mean) row[M] = sqrtf(w[U0 * n + idx]);
      for (int c = P; c < kFpCols; ++c) row[c] = 0.f;
    }
  }
  if (i >= M) return;

  constexpr double inv_s2d = 1.0 / ((double)kSigmaG * (double)kSigmaG);
  const float inv_s2 = (float)inv_s2d, nrm = 0.3989422804014327f / kSigmaG;
  if (tid == 0) {
    const double al = (double)A.alpha[e] * 0.017453292519943295, ca = cos(al), sa = sin(al), c0 = (N - 1) * 0.5;
    const int ci = (A.group ? A.group[e] * M : 0) + i;  // the epoch's own star's source
    XY[0] = c0 + ss * (ca * (double)A.cx[ci] - sa * (double)A.cy[ci] + (double)A.dx[e]);
    XY[1] = c0 + ss * (sa * (double)A.cx[ci] + ca * (double)A.cy[ci] + (double)A.dy[e]);
    XY[2] = ca;
    XY[3] = sa;
    WIN[0] = WIN[2] = N;
    WIN[1] = WIN[3] = -1;
  }
  __syncthreads();
  const double Xd = XY[0], Yd = XY[1];
  auto gauss = [&](int v, double X) {
    const float t = (float)((double)v - X);
    return nrm * expf(-0.5f * t * t * inv_s2);
  };
  {  // the entries kept: not below kFpCut of the table's peak (the entry next to the source, or the border's)
    const double rx = fmin(fmax(rint(Xd), 0.0), (double)(N - 1)), ry = fmin(fmax(rint(Yd), 0.0), (double)(N - 1));
    const float cutx = kFpCut * gauss((int)rx, Xd), cuty = kFpCut * gauss((int)ry, Yd);
    for (int v = tid; v < N; v += kFpThreads) {
      const float gx = gauss(v, Xd), gy = gauss(v, Yd);
      if (gx > 0.f && gx >= cutx) {
        atomicMin(&WIN[0], v);
        atomicMax(&WIN[1], v);
      }
      if (gy > 0.f && gy >= cuty) {
        atomicMin(&WIN[2], v);
        atomicMax(&WIN[3], v);
      }
    }
  }
  __syncthreads();
  const int lox = WIN[0], hix = min(WIN[1], lox + kFpSpan - 1), loy = WIN[2], hiy = min(WIN[3], loy + kFpSpan - 1);
  const bool empty = lox > hix || loy > hiy;  // the source does not reach the grid: zero columns
  // block-summed tables, entry t + ss - 1 for t = -(ss - 1) .. N - 1: sum_s g[t + s] over the entries kept
  for (int k = tid; k < N + ss - 1; k += kFpThreads) {
    float sx = 0.f, sdx = 0.f, sy = 0.f, sdy = 0.f;
    for (int s = 0; s < ss; ++s) {
      const int v = k - (ss - 1) + s;
      if (v >= lox && v <= hix) {
        const float g = gauss(v, Xd);
        sx += g;
        sdx += g * (float)((double)v - Xd) * inv_s2;
      }
      if (v >= loy && v <= hiy) {
        const float g = gauss(v, Yd);
        sy += g;
        sdy += g * (float)((double)v - Yd) * inv_s2;
      }
    }
    GXS[k] = sx;
    DGXS[k] = sdx;
    GYS[k] = sy;
    DGYS[k] = sdy;
  }
  const int c = (N - 1) / 2;  // zero lag of conv_same
  // PSF rows this band's column pass reads: p = u + c - u' for u in the band's rows, u' in [loy, hiy]
  const int p0 = max(0, ss * U0 + c - hiy), p1 = min(N - 1, ss * (U1 - 1) + ss - 1 + c - loy);
  const int np = empty ? 0 : max(0, p1 - p0 + 1);  // <= ss kFpBand + kFpSpan - 1
  __syncthreads();
  const float *psf = A.psf + (size_t)e * N * N;
  const bool cpos = A.positions != 0, pos = cpos || A.shifts;  // the derivative passes; the c columns
  for (int idx = tid; idx < np * n; idx += kFpThreads) {  // row pass, block-summed over v
    const int pr = idx / n, V = idx % n;
    const float *kr = psf + (size_t)(p0 + pr) * N;
    const int qa = max(0, ss * V + c - hix), qb = min(N - 1, ss * V + c - lox + ss - 1);
    const int tb = ss * V + c + ss - 1;  // table entry of tap q: tb - q
    float rg = 0.f, rd = 0.f;
    for (int q = qa; q <= qb; ++q) {
      const float k = kr[q];
      rg = fmaf(k, GXS[tb - q], rg);
      if (pos) rd = fmaf(k, DGXS[tb - q], rd);
    }
    RG[idx] = rg;
    RD[idx] = rd;
  }
  __syncthreads();
  const float ca = (float)XY[2], sa = (float)XY[3], fs = (float)ss;
  const float amp = A.a[(size_t)e * M + i];
  for (int idx = tid; idx < (U1 - U0) * n; idx += kFpThreads) {  // column pass, block-summed over u, and the mix
    const int U = U0 + idx / n, V = idx % n;
    float t = 0.f, gX = 0.f, gY = 0.f;
    if (!empty) {
      const int pa = max(0, ss * U + c - hiy), pb = min(N - 1, ss * U + c - loy + ss - 1);
      const int tb = ss * U + c + ss - 1;
      for (int p = pa; p <= pb; ++p) {
        const float rg = RG[(p - p0) * n + V], gy = GYS[tb - p];
        t = fmaf(gy, rg, t);
        if (pos) {
          gX = fmaf(gy, RD[(p - p0) * n + V], gX);
          gY = fmaf(DGYS[tb - p], rg, gY);
        }
      }
    }
    const int px = U * n + V;
    const float sw = sqrtf(w[px]);
    float *row = slab + (size_t)px * kFpCols;
    row[i] = sw * t;
    if (cpos) {
      row[Lp + i] = sw * amp * fs * (ca * gX + sa * gY);
      row[Lp + M + i] = sw * amp * fs * (ca * gY - sa * gX);
    }
    if (A.shifts) {
      float *g = A.gsh + ((size_t)b * nn + px) * (2 * M) + 2 * i;
      g[0] = amp * fs * gX;
      g[1] = amp * fs * gY;
    }
  }
}


typedef float fp_f32x16 __attribute__((ext_vector_type(16)));

// one workgroup (four waves) per epoch
__global__ __launch_bounds__(kFpThreads) void joint_fisher_gram_kernel(FisherGramArgs A) {
  __shared__ double PART[kFpThreads / 64][kFpCols * kFpCols];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float *T = A.slab + (size_t)b * A.nn * kFpCols;
  const int total = A.nn * kFpCols;
  const int steps = (A.nn + 1) / 2;            // two pixels (64 floats: one 256-byte row) per matrix instruction
  const int iters = (steps + 15) / 16;         // sixteen interleaved streams: four waves x four accumulators
  auto ld = [&](int step) {
    const int idx = step * 64 + lane;
    return idx < total ? T[idx] : 0.f;
  };
  double d[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) d[r] = 0.0;
  for (int t0 = 0; t0 < iters; t0 += 64) {  // 64 steps = 128 pixels per accumulator, then into float64
    fp_f32x16 acc0, acc1, acc2, acc3;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = acc2[r] = acc3[r] = 0.f;
    const int t1 = min(iters, t0 + 64);
    for (int t = t0; t < t1; ++t) {
      const int s = t * 16 + wv * 4;
      const float v0 = ld(s), v1 = ld(s + 1), v2 = ld(s + 2), v3 = ld(s + 3);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, v0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, v1, acc1, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(v2, v2, acc2, 0, 0, 0);
      acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(v3, v3, acc3, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) d[r] += ((double)acc0[r] + (double)acc1[r]) + ((double)acc2[r] + (double)acc3[r]);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {  // C/D map of the 32 x 32 forms
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), col = lane & 31;
    PART[wv][row * kFpCols + col] = d[r];
  }
  __syncthreads();
  double *Fo = A.Fd + (size_t)b * kFpCols * kFpCols;
  for (int k = tid; k < kFpCols * kFpCols; k += kFpThreads) Fo[k] = ((PART[0][k] + PART[1][k]) + PART[2][k]) + PART[3][k];
}


// lower Cholesky factor of the m x m matrix S (row stride ld) into L, pivots against kFpPivot times the diagonal; then
// L^-1 into Li.  One thread.
template <int K>
__device__ bool fp_cholesky(const double (*S)[K], int m, double (*L)[K], double (*Li)[K]) {
  for (int r = 0; r < m; ++r)
    for (int c = 0; c <= r; ++c) {
      double s = S[r][c];
      for (int k = 0; k < c; ++k) s -= L[r][k] * L[c][k];
      if (r == c) {
        if (!(s > kFpPivot * S[r][r])) return false;
        L[r][r] = sqrt(s);
      } else {
        L[r][c] = s / L[c][c];
      }
    }
  for (int c = 0; c < m; ++c) {
    Li[c][c] = 1.0 / L[c][c];
    for (int r = c + 1; r < m; ++r) {
      double s = 0.0;
      for (int k = c; k < r; ++k) s += L[r][k] * Li[k][c];
      Li[r][c] = -s / L[r][r];
    }
  }
  return true;
}

// one workgroup per epoch: F_local, F_cross out; the local factorisation, B_e and F_x^T B_e.  KL: the capacity of the local
// block (kFpLocal, or kFpLocalShifts with dx_e, dy_e), also the stride of Binv and B
template <int KL>
__global__ __launch_bounds__(kFpThreads) void joint_fisher_arrow_local_kernel(FisherArrowArgs A) {
  __shared__ double Fl[KL][KL], Fr[KL][KL], Ld[KL][KL], Li[KL][KL];
  __shared__ double Inv[KL][KL], Fx[KL][kFpShared], Bs[KL][kFpShared];
  __shared__ int IDX[KL], MM[2];
  const int e = blockIdx.x, tid = threadIdx.x, Lp = A.Lp, Sh = A.Sh;
  const double *F = A.Fd + (size_t)e * kFpCols * kFpCols;
  for (int k = tid; k < Lp * Lp; k += kFpThreads) {
    const int r = k / Lp, c = k % Lp;
    Fl[r][c] = F[r * kFpCols + c];
    A.F_local[(size_t)e * Lp * Lp + k] = (float)Fl[r][c];
  }
  for (int k = tid; k < Lp * Sh; k += kFpThreads) {
    const int r = k / Sh, c = k % Sh;
    Fx[r][c] = F[r * kFpCols + Lp + c];
    A.F_cross[(size_t)e * Lp * Sh + k] = (float)Fx[r][c];
  }
  __syncthreads();
  if (tid == 0) {
    int m = 0;
    for (int r = 0; r < Lp; ++r)
      if (Fl[r][r] > 0.0) IDX[m++] = r;
    for (int r = 0; r < m; ++r)
      for (int c = 0; c < m; ++c) Fr[r][c] = Fl[IDX[r]][IDX[c]];
    MM[0] = m;
    MM[1] = fp_cholesky<KL>(Fr, m, Ld, Li) ? 1 : 0;
    A.ok[e] = MM[1];
  }
  __syncthreads();
  const int m = MM[0];
  const bool ok = MM[1] != 0;
  double *Bo = A.B + (size_t)e * KL * kFpShared, *Io = A.Binv + (size_t)e * KL * KL;
  double *Go = A.G + (size_t)e * kFpShared * kFpShared;
  for (int k = tid; k < KL * KL; k += kFpThreads) Io[k] = 0.0;
  for (int k = tid; k < KL * kFpShared; k += kFpThreads) Bo[k] = 0.0;
  for (int k = tid; k < kFpShared * kFpShared; k += kFpThreads) Go[k] = 0.0;
  if (!ok) return;
  __syncthreads();
  if (tid < m * m) {  // F_loc^-1 = L^-T L^-1
    const int r = tid / m, c = tid % m;
    double s = 0.0;
    for (int k = (r > c ? r : c); k < m; ++k) s += Li[k][r] * Li[k][c];
    Inv[r][c] = s;
    Io[IDX[r] * KL + IDX[c]] = s;
  }
  __syncthreads();
  if (tid < m * Sh) {
    const int r = tid / Sh, c = tid % Sh;
    double s = 0.0;
    for (int k = 0; k < m; ++k) s += Inv[r][k] * Fx[IDX[k]][c];
    Bs[r][c] = s;
    Bo[IDX[r] * kFpShared + c] = s;
  }
  __syncthreads();
  if (tid < Sh * Sh) {
    const int r = tid / Sh, c = tid % Sh;
    double s = 0.0;
    for (int k = 0; k < m; ++k) s += Fx[IDX[k]][r] * Bs[k][c];
    Go[r * kFpShared + c] = s;
  }
}

// one workgroup: the sums over the epochs in epoch order, S and its inverse
__global__ __launch_bounds__(kFpThreads) void joint_fisher_arrow_shared_kernel(FisherArrowArgs A) {
  __shared__ double Fc[kFpShared][kFpShared], Sd[kFpShared][kFpShared], Sr[kFpShared][kFpShared];
  __shared__ double Ld[kFpShared][kFpShared], Li[kFpShared][kFpShared];
  __shared__ int IDX[kFpShared], MM[2];
  const int tid = threadIdx.x, Lp = A.Lp, Sh = A.Sh, M = A.M;
  if (A.gstart) {  // a batch: no shared block, and every star's verdict over its own epochs
    for (int g = tid; g < A.stars; g += kFpThreads) {
      int all = 1;
      for (int e = A.gstart[g]; e < A.gstart[g + 1]; ++e) all &= A.ok[e];
      A.ok[A.E + g] = all;
    }
    return;
  }
  if (tid < Sh * Sh) {
    const int r = tid / Sh, c = tid % Sh;
    double f = 0.0, g = 0.0;
    for (int e = 0; e < A.E; ++e) {
      f += A.Fd[(size_t)e * kFpCols * kFpCols + (Lp + r) * kFpCols + Lp + c];
      g += A.G[(size_t)e * kFpShared * kFpShared + r * kFpShared + c];
    }
    if (r == c && A.prior) {
      const double sp = (double)A.prior[(r < M ? M + r : 3 * M + (r - M))];
      f += 1.0 / (sp * sp);
    }
    Fc[r][c] = f;
    Sd[r][c] = f - g;
    A.F_shared[tid] = (float)f;
  }
  __syncthreads();
  if (tid == 0) {
    int all = 1;
    for (int e = 0; e < A.E; ++e) all &= A.ok[e];
    int m = 0;
    for (int r = 0; r < Sh; ++r)
      if (Fc[r][r] > 0.0) IDX[m++] = r;
    for (int r = 0; r < m; ++r)
      for (int c = 0; c < m; ++c) Sr[r][c] = Sd[IDX[r]][IDX[c]];
    if (all && !fp_cholesky<kFpShared>(Sr, m, Ld, Li)) all = 0;
    MM[0] = m;
    MM[1] = all;
    A.ok[A.E] = all;
  }
  __syncthreads();
  const int m = MM[0];
  const bool ok = MM[1] != 0;
  const float nan = __builtin_nanf("");
  for (int k = tid; k < kFpShared * kFpShared; k += kFpThreads) A.Ccc[k] = 0.0;
  if (tid < Sh * Sh) A.C_shared[tid] = ok ? 0.f : nan;
  if (tid < Sh) A.sigma_c[tid] = ok ? __builtin_inff() : nan;
  __syncthreads();
  if (ok && tid < m * m) {
    const int r = tid / m, c = tid % m;
    double s = 0.0;
    for (int k = (r > c ? r : c); k < m; ++k) s += Li[k][r] * Li[k][c];
    A.Ccc[IDX[r] * kFpShared + IDX[c]] = s;
    A.C_shared[IDX[r] * Sh + IDX[c]] = (float)s;
    if (r == c) A.sigma_c[IDX[r]] = (float)sqrt(s);
  }
}

// one workgroup per epoch: C_x = -B C_cc, C_loc = F_loc^-1 + B C_cc B^T, the local sigmas
template <int KL>
__global__ __launch_bounds__(kFpThreads) void joint_fisher_arrow_back_kernel(FisherArrowArgs A) {
  __shared__ double Cx[KL][kFpShared];
  const int e = blockIdx.x, tid = threadIdx.x, Lp = A.Lp, Sh = A.Sh, M = A.M;
  const bool ok = A.ok[A.E + (A.group ? A.group[e] : 0)] != 0;  // the whole solve's verdict, in a batch the epoch's star's
  const float nan = __builtin_nanf("");
  const double *B = A.B + (size_t)e * KL * kFpShared, *Inv = A.Binv + (size_t)e * KL * KL;
  if (tid < Lp * Sh) {
    const int r = tid / Sh, c = tid % Sh;
    double s = 0.0;
    for (int k = 0; k < Sh; ++k) s += B[r * kFpShared + k] * A.Ccc[k * kFpShared + c];
    Cx[r][c] = -s;
    A.C_cross[(size_t)e * Lp * Sh + tid] = ok ? (float)(-s) : nan;
  }
  __syncthreads();
  if (tid < Lp * Lp) {
    const int r = tid / Lp, c = tid % Lp;
    double s = Inv[r * KL + c];
    for (int k = 0; k < Sh; ++k) s -= Cx[r][k] * B[c * kFpShared + k];
    A.C_local[(size_t)e * Lp * Lp + tid] = ok ? (float)s : nan;
    if (r == c) {
      const bool out = !(A.Fd[(size_t)e * kFpCols * kFpCols + r * kFpCols + r] > 0.0);
      const float sg = !ok ? nan : (out ? __builtin_inff() : (float)sqrt(s));
      if (r < M) A.sigma_a[(size_t)e * M + r]  = sg;
      else if (A.shifts && r >= Lp - 2) (r == Lp - 2 ? A.sigma_dx : A.sigma_dy)[e] = sg;
      else A.sigma_mean[e] = sg;
    }
  }
}

#endif  // LC_FISHER_POSITIONS_KERNELS

}  // namespace lc
