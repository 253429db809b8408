// PSF-fit kernels at subsampling 1 above the 16 x 16 fixture size, a translation unit of their own: the kernels of psf_batch.hip
// are what they were (tests/test_psf_budget_isa_cpu.py holds that file to its kernels and their registers).
#undef LC_STAMPS                   // (the clock stamps of the diagnostic build belong to psf_batch.hip)
#define LC_KERNEL_TEMPLATES_ONLY   // the headers' kernels that are no templates are psf_batch.hip's
#include "psf_variants.h"

namespace lc {

const PsfVariant *find_variant_ss1(int n) {
  static const PsfVariant table[] = {
      make_variant<PsfCfg<32, 1, 4, 8, true>>(),    // n = 32
      // n = 64: V of the one-wave layout is [SG][N][n + 3] with n = N and does not fit the LDS at any SG it takes (a
      // multiple of 8); the block-synchronised layout of the N = 128 kernel instead
      make_variant<PsfCfg<64, 1, 16, 1>>(),
  };
  for (const auto &v : table)
    if (v.n == n) return &v;
  return nullptr;
}

noise_fn find_noise_kernel_ss1(int N) {
  if (N == 32) return psf_noise_accumulate_kernel<32, 1>;
  if (N == 64) return psf_noise_accumulate_kernel<64, 1>;
  return nullptr;
}

}  // namespace lc
