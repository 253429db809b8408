// Flux covariance of the joint fit from the full Fisher information (lc_joint_fisher_flux_cov), gfx950.
//
// With only the fluxes free the model is linear in a and the loss is 1/2 sum w r^2, so the Fisher information is the exact
// Hessian, independent of a and block diagonal over the epochs:
//   F_e[i][j] = sum_pix w T_{e,i} T_{e,j},   C_e = F_e^-1,   sigma_{e,i} = sqrt(C_e[i][i])
// with T_{e,i} the unit-flux model of source i in epoch e.  The epoch kernels' template mode (JointArgs::tmpl) leaves
// sqrt(w) T_{e,i} in a slab [b][M][n*n]; this kernel forms the M (M + 1) / 2 products of one epoch per workgroup (fp32 within
// a thread, fp64 across the threads) and solves the block by an fp64 Cholesky factorisation.
//   * a source with F_ii = 0 (no weighted pixel of its template is non-zero: outside the stamp, or masked) gets sigma = +inf
//     and a zero row / column of C; the block is solved without it (the diagonal form returns 1 / sqrt(0) for it too);
//   * a pivot of the factorisation that is not above kFisherPivot times its diagonal entry (the source's template explained
//     by the others' to 1 part in 10^6: its flux is not determined apart from theirs) makes C and sigma of that epoch NaN.
#pragma once
#include "joint_kernels.h"

namespace lc {

constexpr int kFisherThreads = 256;
constexpr int kFisherPairs = kMaxSources * (kMaxSources + 1) / 2;
constexpr double kFisherPivot = 1e-6;

struct FisherCovArgs {
  const float *T;   // [b][M][nn] sqrt(w) T of the launch's epochs
  int M, nn;
  float *F, *C;     // [b][M][M] (each may be null)
  float *sigma;     // [b][M]
};

__global__ __launch_bounds__(kFisherThreads) void joint_fisher_cov_kernel(FisherCovArgs A) {
  __shared__ float PART[kFisherPairs][kFisherThreads];  // every thread's fp32 partial products
  __shared__ double Fd[kMaxSources][kMaxSources], Ld[kMaxSources][kMaxSources], Li[kMaxSources][kMaxSources];
  __shared__ int IDX[kMaxSources];
  const int b = blockIdx.x, tid = threadIdx.x, M = A.M, nn = A.nn;
  const float *Te = A.T + (size_t)b * M * nn;
  float acc[kFisherPairs];
#pragma unroll
  for (int k = 0; k < kFisherPairs; ++k) acc[k] = 0.f;
  for (int px = tid; px < nn; px += kFisherThreads) {
    float t[kMaxSources];
#pragma unroll
    for (int i = 0; i < kMaxSources; ++i) t[i] = (i < M) ? Te[(size_t)i * nn + px] : 0.f;
#pragma unroll
    for (int i = 0, k = 0; i < kMaxSources; ++i)
#pragma unroll
      for (int jj = 0; jj <= i; ++jj, ++k) acc[k] = fmaf(t[i], t[jj], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < kFisherPairs; ++k) PART[k][tid] = acc[k];
  __syncthreads();
  if (tid < kFisherPairs) {  // pair k = i (i + 1) / 2 + jj: one thread adds up the threads' partials in a fixed order
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= tid) ++i;
    const int jj = tid - i * (i + 1) / 2;
    if (i < M) {
      double s = 0.0;
      for (int t = 0; t < kFisherThreads; ++t) s += (double)PART[tid][t];
      Fd[i][jj] = s;
      Fd[jj][i] = s;
    }
  }
  __syncthreads();
  if (tid != 0) return;
  float *Fo = A.F ? A.F + (size_t)b * M * M : nullptr, *Co = A.C ? A.C + (size_t)b * M * M : nullptr;
  float *So = A.sigma ? A.sigma + (size_t)b * M : nullptr;
  if (Fo)
    for (int i = 0; i < M; ++i)
      for (int jj = 0; jj < M; ++jj) Fo[i * M + jj] = (float)Fd[i][jj];
  int m = 0;
  for (int i = 0; i < M; ++i)
    if (Fd[i][i] > 0.0) IDX[m++] = i;
  bool ok = true;
  for (int r = 0; r < m && ok; ++r) {  // F restricted to the sources with F_ii > 0 = L L^T
    for (int c = 0; c <= r; ++c) {
      double s = Fd[IDX[r]][IDX[c]];
      for (int k = 0; k < c; ++k) s -= Ld[r][k] * Ld[c][k];
      if (r == c) {
        if (!(s > kFisherPivot * Fd[IDX[r]][IDX[r]])) {
          ok = false;
          break;
        }
        Ld[r][r] = sqrt(s);
      } else {
        Ld[r][c] = s / Ld[c][c];
      }
    }
  }
  if (ok) {  // L^-1 (lower triangular), then C = L^-T L^-1
    for (int c = 0; c < m; ++c) {
      Li[c][c] = 1.0 / Ld[c][c];
      for (int r = c + 1; r < m; ++r) {
        double s = 0.0;
        for (int k = c; k < r; ++k) s += Ld[r][k] * Li[k][c];
        Li[r][c] = -s / Ld[r][r];
      }
    }
  }
  const float nan = __builtin_nanf("");
  if (Co) {
    for (int i = 0; i < M * M; ++i) Co[i] = ok ? 0.f : nan;
    if (ok)
      for (int r = 0; r < m; ++r)
        for (int c = 0; c < m; ++c) {
          double s = 0.0;
          for (int k = (r > c ? r : c); k < m; ++k) s += Li[k][r] * Li[k][c];
          Co[IDX[r] * M + IDX[c]] = (float)s;
        }
  }
  if (So) {
    for (int i = 0; i < M; ++i) So[i] = ok ? __builtin_inff() : nan;
    if (ok)
      for (int r = 0; r < m; ++r) {
        double s = 0.0;
        for (int k = r; k < m; ++k) s += Li[k][r] * Li[k][r];
        So[IDX[r]] = (float)sqrt(s);
      }
  }
}

}  // namespace lc
