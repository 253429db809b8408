// The joint fit's kernel table entries (joint_fit.hip: find_jv, find_ps_kernel), their builders, and the part of the tables
// that is instantiated in a translation unit of its own (joint_fit_ss1.hip: subsampling 1 above 16 x 16).
#pragma once
#include "joint_kernels.h"
#include "joint_ps.h"

typedef void (*epoch_fn)(lc::JointArgs);
typedef void (*update_fn)(lc::JointUpdArgs);
struct JointVariant {
  int n, ss, L;
  epoch_fn ek;
  int e_lds, e_thr;
  update_fn uk;  // null: regulariser + update run as global-memory kernels (joint_gm.h)
  int u_thr, u_lds;
  bool gspec;
  epoch_fn ek_aux;  // plain convolution / spectrum modes of the same pipeline (noise propagation)
  epoch_fn ek_tile = nullptr;  // global-spectrum kernels: the variant whose column passes go through an LDS tile
  int e_lds_tile = 0;
  // global-spectrum kernels: one phase (A, B, C, B', C', D) per launch on a grid (E, parts); [1] / [3] also in the tile build
  epoch_fn ek_phase[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  epoch_fn ek_phase_tile[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int e_lds_lite = 0, e_lds_lite_tile = 0;  // LDS of the column phases and of phase D (JointCfg::LDS_LITE)
  int lpf = 16;                             // lanes per transform (JointCfg::LPF)
  // cluster form (joint_kernels.h, PHASE = 7): several workgroups per epoch in ONE launch, spectrum in the global scratch;
  // a build of its own beside an LDS-spectrum kernel (same N, SS, L: same spectra)
  epoch_fn ek_cluster = nullptr;
  int cl_lds = 0, cl_thr = 0, cl_lpf = 16;
  // batched star photometry with a background grid per star (lc_joint_create_groups_background): the epoch kernel that reads
  // its epoch's star (JointArgs::group) and the single-workgroup update over the stars' views
  epoch_fn ek_grp = nullptr;
  void (*uk_grp)(const lc::JointUpdArgs *) = nullptr;
  // the template mode (lc_joint_fisher_flux_cov): builds of ek (LDS e_lds) and ek_grp that also store the weighted templates
  epoch_fn ek_tmpl = nullptr, ek_grp_tmpl = nullptr;
};

typedef void (*ps_fn)(lc::JointPsArgs);

// n x n stamps at subsampling 1, n > 16 (null / *fn untouched: none instantiated)
const JointVariant *find_jv_ss1(int n);
void find_ps_kernel_ss1(int N, bool persist, bool tmpl, ps_fn *fn, int *lds);

namespace lc {
namespace {

// BG: also the per-star background forms (lc_joint_create_groups_background) - the sizes of its scope, n <= 32
template <int N, int SS, int L, int PX, int NW, int LPF = 16, bool BG = true>
JointVariant make_jv() {
  typedef JointCfg<N, SS, L, NW, false, LPF> C;
  JointVariant v{C::n, SS, L, joint_epoch_kernel<C>, C::LDS_BYTES, C::NTHR, joint_update_kernel<N, PX>, N * N / PX,
                 (int)(StarletLds<N>::FLOATS * sizeof(float)), false, joint_epoch_kernel<C, true>};
  v.ek_tmpl = joint_epoch_kernel<C, false, 0, false, true>;
  if constexpr (BG) {
    v.ek_grp = joint_epoch_kernel<C, false, 0, true>;
    v.uk_grp = joint_update_groups_uk_kernel<N, PX>;
    v.ek_grp_tmpl = joint_epoch_kernel<C, false, 0, true, true>;
  }
  return v;
}
// ... with the cluster form beside it: four-wave workgroups (one wave per SIMD), spectrum in the global scratch
template <int N, int SS, int L, int PX, int NW, int LPF, int CNW, int CLPF>
JointVariant make_jv_cl() {
  // (no per-star background form: n = 64 is outside its scope - the one-star fit runs the cluster form there)
  JointVariant v = make_jv<N, SS, L, PX, NW, LPF, false>();
  typedef JointCfg<N, SS, L, CNW, true, CLPF> CC;
  v.ek_cluster = joint_epoch_kernel<CC, false, 7>;
  v.cl_lds = CC::LDS_BYTES;
  v.cl_thr = CC::NTHR;
  v.cl_lpf = CLPF;
  return v;
}
// stamp sizes beside the tuned ones (any multiple of 8 up to 64 at ss = 2): the same epoch kernel at that N, regulariser and
// update as the run-time-N multi-block kernels (joint_gm.h) instead of a single-workgroup kernel built per size
template <int N, int SS, int L, int NW, int LPF = 16>
JointVariant make_jv_plain() {
  typedef JointCfg<N, SS, L, NW, false, LPF> C;
  JointVariant v{C::n, SS, L, joint_epoch_kernel<C>, C::LDS_BYTES, C::NTHR, nullptr, 0, 0, false, joint_epoch_kernel<C, true>};
  v.ek_tmpl = joint_epoch_kernel<C, false, 0, false, true>;
  return v;
}

}  // namespace
}  // namespace lc
