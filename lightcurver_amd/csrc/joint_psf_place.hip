// The placement kernel of lc_joint_create_psf (joint_psf_place.h) and its launcher.
#define LC_PSF_PLACE_KERNELS
#include "joint_psf_place.h"

namespace lc {

void launch_psf_place(int E, int P, int N, const float *stamp, float *grid, hipStream_t q) {
  hipLaunchKernelGGL(joint_psf_place_kernel, dim3((unsigned)((N * N + kPlaceThreads - 1) / kPlaceThreads), (unsigned)E),
                     dim3(kPlaceThreads), 0, q, P, N, stamp, grid);
}

}  // namespace lc
