// The kernels of lc_joint_fisher_positions (joint_fisher_positions.h) and their launchers, a translation unit of their own.
#define LC_FISHER_POSITIONS_KERNELS
#include "joint_fisher_positions.h"

namespace lc {

void launch_fisher_tmpl(const FisherTmplArgs &A, int bands, int sources, int epochs, size_t lds, hipStream_t q) {
  hipLaunchKernelGGL(joint_fisher_tmpl_kernel, dim3(bands, sources, epochs), dim3(kFpThreads), lds, q, A);
}

void launch_fisher_gram(const FisherGramArgs &A, int epochs, hipStream_t q) {
  hipLaunchKernelGGL(joint_fisher_gram_kernel, dim3(epochs), dim3(kFpThreads), 0, q, A);
}

template <int KL>
static void launch_arrow(const FisherArrowArgs &A, hipStream_t q) {
  hipLaunchKernelGGL(joint_fisher_arrow_local_kernel<KL>, dim3(A.E), dim3(kFpThreads), 0, q, A);
  hipLaunchKernelGGL(joint_fisher_arrow_shared_kernel, dim3(1), dim3(kFpThreads), 0, q, A);
  hipLaunchKernelGGL(joint_fisher_arrow_back_kernel<KL>, dim3(A.E), dim3(kFpThreads), 0, q, A);
}

void launch_fisher_arrow(const FisherArrowArgs &A, hipStream_t q) {
  if (A.shifts) launch_arrow<kFpLocalShifts>(A, q);
  else launch_arrow<kFpLocal>(A, q);
}

}  // namespace lc
