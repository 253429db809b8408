// Detection, de-blending, clean and segmentation of the sources of a star stamp: what the reference gets from
// sep.extract(data, thresh=3, err=noisemap, minarea=15, segmentation_map=True, deblend_cont=0.001) inside
// mask_surrounding_stars (lightcurver/processes/psf_modelling.py:35-61), frozen as the SPEC of DESIGN.md §5 "Source
// masking".  The per-pixel stage is float32 with every operation rounded on its own, every sum that decides something
// is an exact 64-bit integer sum of the 2^-20 fixed point, the per-object scalars are float64, so the result is bit for
// bit that of the SPEC's NumPy restatement (tests/_segment.py).
//
// One workgroup per stamp, every plane in LDS (15 n^2 bytes: 60 KiB at n = 64): the S/N image, a 64-bit accumulator
// per pixel (indexed by an island's first pixel), the island labels and the tree node that owns each pixel.  Connected
// components by min-label propagation with one pointer jump per sweep; the de-blending recursion is a work list of tree
// nodes the whole workgroup walks, the pixels left over by a split are assigned bottom-up afterwards: deblend_tree.h,
// written for a rectangular box; the shape and the wing of clean are clean_shape.h, which deblend.hip shares.  No
// device-memory flags or atomics: every atomic is on LDS.
#pragma clang fp contract(off)  // the SPEC fixes every rounding: no fused multiply-adds, on the device or the host

#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "clean_shape.h"
#include "deblend_tree.h"
#include "device_call.h"
#include "lc_common.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kSegThreads = 256;
static_assert(kSegThreads == kTreeThreads, "segment_kernel's workgroup walks the tree");
constexpr int kSegMinN = 8, kSegMaxN = 64;
constexpr int kSegObjCap = kTreeLeafCap;  // objects before clean

__host__ __device__ constexpr size_t seg_plane_bytes(int n) { return (size_t)n * n * kTreeLdsPerPixel; }

struct SegArgs {
  int K, n, minarea, nthresh, nroot, clean;
  float thresh;
  double cont;
  const float *data, *noise;
  uint8_t *mask;
  int32_t *segmap, *nobj, *status;
  float *xy;
};

// the objects of a stamp, beside the tree (TreeShared)
struct SegShared {
  int nobj, central;
  long long ob_sum[kSegObjCap][6];  // q, q x, q y, q x^2, q y^2, q x y
  int ob_npix[kSegObjCap], ob_cnt[kSegObjCap];
  unsigned ob_kth[kSegObjCap];
  CleanShape shape[kSegObjCap];
  int target[kSegObjCap], final_index[kSegObjCap], obj_of[kSegObjCap];
  float out_xy[kSegObjCap][2];
};

__global__ __launch_bounds__(kSegThreads) void segment_kernel(SegArgs A) {
  extern __shared__ __align__(16) unsigned char seg_lds[];
  __shared__ TreeShared T;
  __shared__ SegShared S;
  const int n = A.n, np = n * n, tid = threadIdx.x, k = blockIdx.x;
  const TreeBox B(seg_lds, np, n, n);
  long long *acc = B.acc;
  float *snr = B.snr;
  uint16_t *lab = B.lab;
  uint8_t *L = B.L;
  const size_t off = (size_t)k * np;
  const float th0 = A.thresh;

  // ---- per-pixel stage: w = 1 / (s s), the 3 x 3 filter, snr (float32, every operation rounded on its own) ----
  {
    float *W = (float *)acc, *DW = W + np;
    for (int p = tid; p < np; p += kSegThreads) {
      const float d = A.data[off + p], s = A.noise[off + p];
      const bool ok = __builtin_isfinite(d) && __builtin_isfinite(s) && s > 0.f;
      float w = 0.f, dw = 0.f;
      if (ok) {
        w = 1.0f / (s * s);
        dw = d * w;
      }
      W[p] = w;
      DW[p] = dw;
    }
    if (tid == 0) {
      T.status = 0;
      T.nnodes = 0;
      T.nleaf = 0;
      S.nobj = 0;
      S.central = -1;
    }
    __syncthreads();
    int bad = 0;
    for (int p = tid; p < np; p += kSegThreads) {
      const int i = p / n, j = p - i * n;
      float num = 0.f, den2 = 0.f;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int y = i + dy, x = j + dx;
          const bool in = y >= 0 && y < n && x >= 0 && x < n;
          const float kf = (float)((2 - (dy < 0 ? -dy : dy)) * (2 - (dx < 0 ? -dx : dx)));
          const float v = in ? DW[y * n + x] : 0.f, ww = in ? W[y * n + x] : 0.f;
          num = num + kf * v;
          den2 = den2 + (kf * kf) * ww;
        }
      const float r = den2 > 0.f ? num / sqrtf(den2) : 0.f;
      snr[p] = r;
      L[p] = (uint8_t)kTreeNoNode;
      bad |= (r > th0 && !(r < kTreeSnrLimit)) ? 1 : 0;
    }
    // (W and DW share the accumulator plane: the barrier below comes before anything else is written there)
    if (__syncthreads_or(bad)) {
      if (tid == 0) T.status = 3;
      __syncthreads();
    }
  }

  // ---- the groups as the first nodes, the de-blending trees under them, the leaves = objects before clean ----
  if (T.status == 0) {
    const int kk = tree_islands(kTreeNoNode, th0, B, T);
    if (T.status == 0 && kk > 0) tree_make_children<true>(-1, th0, 0, 0, A.cont, A.nthresh, A.minarea, B, T);
  }
  tree_walk(B, T);
  tree_leaves(B, T);

  // ---- per-object sums, shapes, clean, the central object ----
  const bool have = T.status == 0 && T.nleaf > 0;
  if (have) {
    const int nleaf = T.nleaf;
    if (tid < nleaf) {
      for (int c = 0; c < 6; ++c) S.ob_sum[tid][c] = 0;
      S.ob_npix[tid] = 0;
      S.ob_kth[tid] = 0;
      S.target[tid] = -1;
    }
    __syncthreads();
    for (int p = tid; p < np; p += kSegThreads) {
      const unsigned node = L[p];
      unsigned rk = kTreeNone;
      if (node != kTreeNoNode) {
        rk = (unsigned)T.nd_rank[node];
        const int i = p / n, j = p - i * n;
        const long long q = tree_q(snr[p]);
        unsigned long long *s = (unsigned long long *)S.ob_sum[rk];
        atomicAdd(s + 0, (unsigned long long)q);
        atomicAdd(s + 1, (unsigned long long)(q * j));
        atomicAdd(s + 2, (unsigned long long)(q * i));
        atomicAdd(s + 3, (unsigned long long)(q * j * j));
        atomicAdd(s + 4, (unsigned long long)(q * i * i));
        atomicAdd(s + 5, (unsigned long long)(q * j * i));
        atomicAdd(&S.ob_npix[rk], 1);
      }
      lab[p] = (uint16_t)rk;
    }
    __syncthreads();
    if (A.clean && nleaf >= 2) {
      // the minarea-th largest snr of every object at once: its bits, built from the top bit down
      for (int bit = 30; bit >= 0; --bit) {
        if (tid < nleaf) S.ob_cnt[tid] = 0;
        __syncthreads();
        for (int p = tid; p < np; p += kSegThreads) {
          const unsigned rk = lab[p];
          if (rk == kTreeNone) continue;
          if (__float_as_uint(snr[p]) >= (S.ob_kth[rk] | (1u << bit))) atomicAdd(&S.ob_cnt[rk], 1);
        }
        __syncthreads();
        if (tid < nleaf && S.ob_cnt[tid] >= A.minarea) S.ob_kth[tid] |= 1u << bit;
        __syncthreads();
      }
      if (tid < nleaf) {
        const long long *s = S.ob_sum[tid];
        S.shape[tid] = clean_shape((double)s[0], (double)s[1], (double)s[2], (double)s[3], (double)s[4], (double)s[5],
                                   kTreeFix, S.ob_npix[tid], A.minarea, S.ob_kth[tid], th0, 0.0, 0.0);
      }
      __syncthreads();
      if (tid == 0) {
        // faintest first (ties: the lower index first); the shapes are those of before any merge
        int order[kSegObjCap];
        for (int i = 0; i < nleaf; ++i) {
          int pos = i;
          while (pos > 0 && S.ob_sum[order[pos - 1]][0] > S.ob_sum[i][0]) {
            order[pos] = order[pos - 1];
            --pos;
          }
          order[pos] = i;
        }
        const double thd = (double)th0;
        for (int oi = 0; oi < nleaf; ++oi) {
          const int i = order[oi];
          double best = 0.0;
          int into = -1;
          for (int j = 0; j < nleaf; ++j) {
            if (j == i || S.target[j] >= 0 || S.ob_sum[j][0] <= S.ob_sum[i][0]) continue;
            const double wing = clean_wing(S.shape[i], S.shape[j], thd);
            if (wing > S.shape[i].mth && wing > best) {
              best = wing;
              into = j;
            }
          }
          S.target[i] = into;
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      int nobj = 0;
      for (int i = 0; i < nleaf; ++i) S.final_index[i] = S.target[i] < 0 ? nobj++ : -1;
      long long fs[kSegObjCap][3];
      for (int r = 0; r < nobj; ++r) fs[r][0] = fs[r][1] = fs[r][2] = 0;
      for (int i = 0; i < nleaf; ++i) {
        int j = i;
        while (S.target[j] >= 0) j = S.target[j];
        const int r = S.final_index[j];
        S.obj_of[i] = r;
        fs[r][0] += S.ob_sum[i][0];
        fs[r][1] += S.ob_sum[i][1];
        fs[r][2] += S.ob_sum[i][2];
      }
      const double c = (double)(n - 1) / 2.0;
      double bestd = 0.0;
      int central = -1;
      for (int r = 0; r < nobj; ++r) {
        const double x = (double)fs[r][1] / (double)fs[r][0], y = (double)fs[r][2] / (double)fs[r][0];
        S.out_xy[r][0] = (float)x;
        S.out_xy[r][1] = (float)y;
        const double d2 = (x - c) * (x - c) + (y - c) * (y - c);
        if (r == 0 || d2 < bestd) {
          bestd = d2;
          central = r;
        }
      }
      S.nobj = nobj;
      S.central = central;
    }
    __syncthreads();
  }

  // ---- outputs: defined for every status ----
  const bool fine = T.status == 0;
  const int nobj = fine ? S.nobj : 0, central = S.central;
  for (int p = tid; p < np; p += kSegThreads) {
    int seg = 0;
    if (have && fine && lab[p] != kTreeNone) {
      seg = S.obj_of[lab[p]] + 1;
    }
    A.mask[off + p] = (seg == 0 || seg == central + 1) ? 1 : 0;
    if (A.segmap) A.segmap[off + p] = seg;
  }
  if (A.xy && tid < kSegObjCap) {
    A.xy[((size_t)k * kSegObjCap + tid) * 2 + 0] = tid < nobj ? S.out_xy[tid][0] : 0.f;
    A.xy[((size_t)k * kSegObjCap + tid) * 2 + 1] = tid < nobj ? S.out_xy[tid][1] : 0.f;
  }
  if (tid == 0) {
    if (A.nobj) A.nobj[k] = nobj;
    if (A.status) A.status[k] = T.status;
  }
}

}  // namespace lc

using namespace lc;

extern "C" {

int lc_segment_supported(int n) { return n >= kSegMinN && n <= kSegMaxN ? 1 : 0; }

int lc_segment_stamps(lc_ctx *ctx, int K, int n, const float *data, const float *noisemap, const lc_segment_cfg *cfg,
                      uint8_t *mask, int32_t *segmap, int32_t *nobj, float *xy, int32_t *status, float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  if (K <= 0 || !data || !noisemap || !cfg || !mask) LC_FAIL(ctx, LC_ERR_INVALID, "lc_segment_stamps: invalid argument");
  if (!lc_segment_supported(n)) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_segment_stamps: stamp size outside 8 .. 64");
  if (cfg->clean_param != 1.0f) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_segment_stamps: only clean_param = 1 is built");
  const int nt = cfg->deblend_nthresh;
  if (nt != 4 && nt != 8 && nt != 16 && nt != 32)
    LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_segment_stamps: deblend_nthresh must be 4, 8, 16 or 32");
  if (cfg->minarea < 1) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_segment_stamps: minarea must be at least 1");
  if (!(cfg->thresh > 0.f) || !std::isfinite(cfg->thresh) || !(cfg->deblend_cont >= 0.f) ||
      !std::isfinite(cfg->deblend_cont))
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_segment_stamps: thresh must be positive and deblend_cont non-negative");
  LC_ENTER(ctx);
  const size_t np = (size_t)n * n, tot = (size_t)K * np;
  DeviceCall call(ctx);
  SegArgs A;
  std::memset(&A, 0, sizeof(A));
  A.K = K;
  A.n = n;
  A.minarea = cfg->minarea;
  A.nthresh = nt;
  A.clean = cfg->clean != 0;
  A.thresh = cfg->thresh;
  A.cont = (double)cfg->deblend_cont;
  LC_HIP(ctx, call.upload(data, tot, &A.data));
  LC_HIP(ctx, call.upload(noisemap, tot, &A.noise));
  LC_HIP(ctx, call.result(mask, tot, &A.mask));
  LC_HIP(ctx, call.result(segmap, tot, &A.segmap));
  LC_HIP(ctx, call.result(nobj, (size_t)K, &A.nobj));
  LC_HIP(ctx, call.result(status, (size_t)K, &A.status));
  LC_HIP(ctx, call.result(xy, (size_t)K * kSegObjCap * 2, &A.xy));
  const size_t lds_bytes = seg_plane_bytes(n);
  LC_HIP(ctx, hipFuncSetAttribute((const void *)segment_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes));
  LC_HIP(ctx, call.start());
  hipLaunchKernelGGL(segment_kernel, dim3(K), dim3(kSegThreads), lds_bytes, ctx->stream, A);
  LC_HIP(ctx, hipGetLastError());
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

}  // extern "C"
