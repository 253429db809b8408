// Joint-fit kernels at subsampling 1 above the 16 x 16 fixture size, a translation unit of their own: the kernels of
// joint_fit.hip are what they were (tests/test_psf_budget_isa_cpu.py holds that file to its kernels and their registers).
// The updates of N = 32, 48, 64, 128 are the instantiations the subsampling-2 entries of the same N have there.
#undef LC_STAMPS                   // (the clock stamps of the diagnostic build belong to joint_fit.hip)
#define LC_KERNEL_TEMPLATES_ONLY   // the headers' kernels that are no templates are joint_fit.hip's
#include "joint_variants.h"

using namespace lc;

const JointVariant *find_jv_ss1(int n) {
  static const JointVariant table[] = {
      // An N the subsampling-2 entries have (joint_fit.hip: find_jv) carries the same (L, LPF, waves, update); no FOLD (rows at
      // the grid's own resolution), no per-star background batch (BG = false: its scope stays n <= 32 at ss = 2, n = 16 at 1).
      // N = 24, 40, 56 are multiples of 8 and not of 16: transforms over 8 lanes (fft_device.h), run-time-N update
      make_jv_plain<24, 1, 48, 4, 8>(),                // n = 24: 8-lane transforms of 6 points
      make_jv<32, 1, 48, 4, 16, 16, false>(),          // n = 32
      make_jv_plain<40, 1, 64, 4, 8>(),                // n = 40
      make_jv<48, 1, 96, 4, 8, 16, false>(),           // n = 48
      make_jv_plain<56, 1, 96, 4, 8>(),                // n = 56
      make_jv<64, 1, 96, 8, 16, 16, false>(),          // n = 64
      make_jv_cl<128, 1, 192, 16, 8, 16, 4, 16>(),     // n = 128
  };
  for (const auto &v : table)
    if (v.n == n) return &v;
  return nullptr;
}

void find_ps_kernel_ss1(int N, bool persist, bool tmpl, ps_fn *fn, int *lds) {
#define LC_PS(NN_)                                                                                                      \
  if (N == NN_) {                                                                                                       \
    *fn = persist ? joint_ps_kernel<NN_, 1, true> : (tmpl ? joint_ps_kernel<NN_, 1, false, true> : joint_ps_kernel<NN_, 1, false>); \
    *lds = joint_ps_lds_bytes<NN_, 1>();                                                                                \
  }
  LC_PS(24)
  LC_PS(32)
  LC_PS(40)
  LC_PS(48)
  LC_PS(56)
  LC_PS(64)
  LC_PS(128)
#undef LC_PS
}
