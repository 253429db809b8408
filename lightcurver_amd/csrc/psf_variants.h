// The PSF fit's kernel table entries (psf_batch.hip: find_variant, find_noise_kernel) and the part of the tables that is
// instantiated in a translation unit of its own (psf_batch_ss1.hip: subsampling 1 above 16 x 16).
#pragma once
#include "psf_kernels.h"
#include "psf_noise.h"

namespace lc {

typedef void (*psf_kernel_fn)(PsfArgs);
struct PsfVariant {
  int n, ss;
  psf_kernel_fn fn;
  int nthr, lds_bytes;
  psf_kernel_fn fn_split;  // two workgroups per frame, or null
};

template <class C, bool WITH_SPLIT = false>
PsfVariant make_variant() {
  psf_kernel_fn split = nullptr;
  if constexpr (WITH_SPLIT) split = psf_fit_kernel<C, true>;
  return PsfVariant{C::n, C::SS, psf_fit_kernel<C>, C::NTHR, (int)(C::LDS_FLOATS * sizeof(float)), split};
}

typedef void (*noise_fn)(int, int, const float *, const float *, const float *, float *);

// n x n stamps at subsampling 1, n > 16 (null: none instantiated)
const PsfVariant *find_variant_ss1(int n);
noise_fn find_noise_kernel_ss1(int N);

}  // namespace lc
