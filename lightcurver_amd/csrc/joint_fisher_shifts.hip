// The kernels of the dx_e, dy_e columns of lc_joint_fisher_shifts (joint_fisher_shifts.h) and their launcher.
#define LC_FISHER_SHIFTS_KERNELS
#include "joint_fisher_shifts.h"

namespace lc {

void launch_fisher_shift_cols(const FisherShiftArgs &A, int epochs, hipStream_t q) {
  if (A.h) {
    const int entries = (A.N + A.ss - 1) * 2 * A.N;
    hipLaunchKernelGGL(joint_fisher_shift_field_kernel, dim3((entries + kFpThreads - 1) / kFpThreads, epochs), dim3(kFpThreads),
                       0, q, A);
  }
  const int waves = ((A.n + kFsRows - 1) / kFsRows) * ((A.n + 63) / 64), per = kFpThreads / 64;
  const dim3 grid((waves + per - 1) / per, epochs);
  if (A.ss == 1) hipLaunchKernelGGL(joint_fisher_shift_cols_kernel<1>, grid, dim3(kFpThreads), 0, q, A);
  else hipLaunchKernelGGL(joint_fisher_shift_cols_kernel<2>, grid, dim3(kFpThreads), 0, q, A);
}

}  // namespace lc
