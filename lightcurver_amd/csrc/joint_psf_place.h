// PSF stamps of a side other than the joint fit's grid (SPEC in DESIGN.md section 3): a P x P stamp is placed on the
// N x N grid (N = ss n) with the zero lags of conv_same coinciding, c_P = (P - 1) / 2 on c_N = (N - 1) / 2.  Tap (a, b)
// goes to (a + c_N - c_P, b + c_N - c_P), taps that leave [0, N) are dropped, nothing is renormalised.  For P <= N that
// is the same linear operator; for P > N the N x N window is all the epoch kernels' transforms carry.
// The one function below is the rule: the device placement, and the host cross-check paths of joint_fit.hip
// (LCMI_SPECTRA_HOST, LCMI_NOISE_HOST), which read the stamps at their own size, all go through it.
// The kernel is compiled in joint_psf_place.hip alone (LC_PSF_PLACE_KERNELS); joint_fit.hip calls its launcher.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace lc {

constexpr int kPlaceThreads = 256;

// source index r_s * P + c_s in a P x P stamp of the grid pixel dst = r * N + c (0 <= dst < N * N), or -1 where the grid
// pixel lies outside the stamp
__host__ __device__ inline int psf_place_source(int P, int N, int dst) {
  const int off = (N - 1) / 2 - (P - 1) / 2;
  const int r = dst / N - off, c = dst % N - off;
  return (r >= 0 && r < P && c >= 0 && c < P) ? r * P + c : -1;
}

// enqueues the placement of E stamps (E <= 65535: one row of blocks per epoch) on q
void launch_psf_place(int E, int P, int N, const float *stamp, float *grid, hipStream_t q);

#ifdef LC_PSF_PLACE_KERNELS
// grid[e][r][c] = stamp[e][source of (r, c)] or 0; grid (ceil(N * N / kPlaceThreads), E), one thread per grid pixel
__global__ void joint_psf_place_kernel(int P, int N, const float *stamp, float *grid) {
  const int e = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N * N) return;
  const int s = psf_place_source(P, N, k);
  grid[(size_t)e * N * N + k] = s >= 0 ? stamp[(size_t)e * P * P + s] : 0.f;
}
#endif  // LC_PSF_PLACE_KERNELS

}  // namespace lc
