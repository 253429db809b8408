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
// nodes the whole workgroup walks, the pixels left over by a split are assigned bottom-up afterwards.  No device-memory
// flags or atomics: every atomic is on LDS.
#pragma clang fp contract(off)  // the SPEC fixes every rounding: no fused multiply-adds, on the device or the host

#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_call.h"
#include "lc_common.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kSegThreads = 256;
constexpr int kSegWaves = kSegThreads / 64;
constexpr int kSegMinN = 8, kSegMaxN = 64;
constexpr int kSegObjCap = LC_SEGMENT_MAX_OBJECTS;  // leaves of the de-blending trees of one stamp (objects before clean)
constexpr int kSegNodeCap = 64;  // nodes of those trees, the groups included: the work list
constexpr unsigned kSegNone = 0xFFFFu;
constexpr unsigned kSegNoNode = 0xFFu;
constexpr double kSegFix = 1048576.0;     // 2^20
constexpr float kSegSnrLimit = 65536.0f;  // fixed-point range of a detected pixel

__host__ __device__ constexpr size_t seg_plane_bytes(int n) { return (size_t)n * n * 15; }

struct SegArgs {
  int K, n, minarea, nthresh, nroot, clean;
  float thresh;
  double cont;
  const float *data, *noise;
  uint8_t *mask;
  int32_t *segmap, *nobj, *status;
  float *xy;
};

struct SegShared {
  long long red64[kSegWaves];
  int redi[kSegWaves];
  unsigned redu[kSegWaves];
  // the tree
  double nd_cont[kSegNodeCap];
  float nd_thresh[kSegNodeCap];
  int nd_nthresh[kSegNodeCap], nd_first[kSegNodeCap], nd_nchild[kSegNodeCap], nd_parent[kSegNodeCap];
  int nd_rank[kSegNodeCap], nd_lo[kSegNodeCap], nd_hi[kSegNodeCap];
  int list[kSegNodeCap];
  int nnodes, status, ngood, nleaf, nobj, central;
  // the leaves = objects before clean
  int leaf_node[kSegObjCap];
  unsigned long long lf_key[kSegObjCap];
  int lf_area[kSegObjCap], lf_py[kSegObjCap], lf_px[kSegObjCap];
  double lf_s2[kSegObjCap];
  long long ob_sum[kSegObjCap][6];  // q, q x, q y, q x^2, q y^2, q x y
  int ob_npix[kSegObjCap], ob_cnt[kSegObjCap];
  unsigned ob_kth[kSegObjCap];
  double sh_mx[kSegObjCap], sh_my[kSegObjCap], sh_a[kSegObjCap], sh_cxx[kSegObjCap], sh_cyy[kSegObjCap],
      sh_cxy[kSegObjCap], sh_unit[kSegObjCap], sh_amp[kSegObjCap], sh_mth[kSegObjCap];
  int target[kSegObjCap], final_index[kSegObjCap], obj_of[kSegObjCap];
  float out_xy[kSegObjCap][2];
};

__device__ __forceinline__ long long seg_q(float v) { return (long long)rint((double)v * kSegFix); }

__device__ __forceinline__ long long seg_sum64(long long v, SegShared &S) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) S.red64[threadIdx.x >> 6] = v;
  __syncthreads();
  long long r = 0;
  for (int w = 0; w < kSegWaves; ++w) r += S.red64[w];
  __syncthreads();
  return r;
}

__device__ __forceinline__ int seg_sumi(int v, SegShared &S) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) S.redi[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
  for (int w = 0; w < kSegWaves; ++w) r += S.redi[w];
  __syncthreads();
  return r;
}

__device__ __forceinline__ unsigned seg_maxu(unsigned v, SegShared &S) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_down((int)v, o, 64));
  if ((threadIdx.x & 63) == 0) S.redu[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned r = 0;
  for (int w = 0; w < kSegWaves; ++w) r = max(r, S.redu[w]);
  __syncthreads();
  return r;
}

// 8-connected islands of {p : L[p] == node and snr[p] > lev}: lab[p] = the island's first pixel in raster order
// (kSegNone outside the set).  Returns the number of islands (0 or 1 without labelling when the set has < 2 pixels).
__device__ int seg_islands(unsigned node, float lev, const float *snr, const uint8_t *L, uint16_t *lab, long long *acc,
                           int n, SegShared &S) {
  const int np = n * n, tid = threadIdx.x;
  int cnt = 0;
  for (int p = tid; p < np; p += kSegThreads) {
    const bool m = L[p] == node && snr[p] > lev;
    lab[p] = m ? (uint16_t)p : (uint16_t)kSegNone;
    cnt += m;
  }
  const int members = seg_sumi(cnt, S);
  if (members == 0) return 0;
  bool converged = members == 1;
  for (int sweep = 0; sweep < np && !converged; ++sweep) {
    int changed = 0;
    for (int p = tid; p < np; p += kSegThreads) {
      const unsigned l = lab[p];
      if (l == kSegNone) continue;
      const int i = p / n, j = p - i * n;
      unsigned m = l;
      for (int y = max(i - 1, 0); y <= min(i + 1, n - 1); ++y)
        for (int x = max(j - 1, 0); x <= min(j + 1, n - 1); ++x) m = min(m, (unsigned)lab[y * n + x]);
      m = min(m, (unsigned)lab[m]);  // a label is a pixel of the same island, whose own label is no larger
      if (m < l) {
        lab[p] = (uint16_t)m;
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) converged = true;
  }
  if (!converged) {
    if (tid == 0) S.status = 2;
    __syncthreads();
    return 0;
  }
  cnt = 0;
  for (int p = tid; p < np; p += kSegThreads)
    if (lab[p] == p) {
      acc[p] = 0;
      ++cnt;
    }
  return seg_sumi(cnt, S);
}

// The islands labelled in lab become child nodes of `parent` (-1: the groups of the stamp) where they pass the
// criterion: at least minarea pixels for a group, flux >= cont * total for a branch; a split needs two of them.
// Returns the number of children made (0: nothing changed).  Sets status 1 when the work list is full.
__device__ int seg_make_children(int parent, float lev, long long qt, long long total, double cont, int nthresh,
                                 const SegArgs &A, const float *snr, uint8_t *L, const uint16_t *lab, long long *acc,
                                 SegShared &S) {
  const int np = A.n * A.n, tid = threadIdx.x;
  const bool top = parent < 0;
  if (tid == 0) S.ngood = 0;
  for (int p = tid; p < np; p += kSegThreads) {
    const unsigned l = lab[p];
    if (l == kSegNone) continue;
    const long long v = top ? 1 : seg_q(snr[p]) - qt;
    atomicAdd((unsigned long long *)&acc[l], (unsigned long long)v);
  }
  __syncthreads();
  const double bar = cont * (double)total;
  for (int p = tid; p < np; p += kSegThreads) {
    if (lab[p] != p) continue;
    const long long f = acc[p];
    const bool good = top ? f >= (long long)A.minarea : (double)f >= bar;
    int slot = kSegNodeCap;
    if (good) slot = atomicAdd(&S.ngood, 1);
    if (slot < kSegNodeCap)
      S.list[slot] = p;
    else
      acc[p] = -1;
  }
  __syncthreads();
  const int ngood = S.ngood, base = S.nnodes;
  if (ngood < (top ? 1 : 2)) return 0;
  if (base + ngood > kSegNodeCap) {
    __syncthreads();
    if (tid == 0) S.status = 1;
    __syncthreads();
    return 0;
  }
  if (tid < ngood) {
    const int p = S.list[tid];
    int rank = 0;
    for (int u = 0; u < ngood; ++u) rank += S.list[u] < p;
    const int id = base + rank;
    const long long f = acc[p];
    S.nd_thresh[id] = lev;
    S.nd_nthresh[id] = top ? nthresh : max(nthresh / 2, 4);
    S.nd_cont[id] = top ? cont : (f > 0 ? bar / (double)f : 0.0);
    S.nd_first[id] = 0;
    S.nd_nchild[id] = 0;
    S.nd_parent[id] = parent;
    acc[p] = id;
  }
  __syncthreads();
  for (int p = tid; p < np; p += kSegThreads) {
    const unsigned l = lab[p];
    if (l == kSegNone) continue;
    const long long c = acc[l];
    if (c >= 0) L[p] = (uint8_t)c;
  }
  if (tid == 0) {
    if (!top) {
      S.nd_first[parent] = base;
      S.nd_nchild[parent] = ngood;
    }
    S.nnodes = base + ngood;
  }
  __syncthreads();
  return ngood;
}

__global__ __launch_bounds__(kSegThreads) void segment_kernel(SegArgs A) {
  extern __shared__ __align__(16) unsigned char seg_lds[];
  __shared__ SegShared S;
  const int n = A.n, np = n * n, tid = threadIdx.x, k = blockIdx.x;
  long long *acc = (long long *)seg_lds;
  float *snr = (float *)(acc + np);
  uint16_t *lab = (uint16_t *)(snr + np);
  uint8_t *L = (uint8_t *)(lab + np);
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
      S.status = 0;
      S.nnodes = 0;
      S.nleaf = 0;
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
      L[p] = (uint8_t)kSegNoNode;
      bad |= (r > th0 && !(r < kSegSnrLimit)) ? 1 : 0;
    }
    // (W and DW share the accumulator plane: the barrier below comes before anything else is written there)
    if (__syncthreads_or(bad)) {
      if (tid == 0) S.status = 3;
      __syncthreads();
    }
  }

  // ---- groups, then the work list of the de-blending trees ----
  if (S.status == 0) {
    const int kk = seg_islands(kSegNoNode, th0, snr, L, lab, acc, n, S);
    if (S.status == 0 && kk > 0)
      seg_make_children(-1, th0, 0, 0, A.cont, A.nthresh, A, snr, L, lab, acc, S);
  }
  for (int x = 0; S.status == 0 && x < S.nnodes; ++x) {
    long long sq = 0;
    int ar = 0;
    unsigned pk = 0;
    for (int p = tid; p < np; p += kSegThreads)
      if (L[p] == x) {
        sq += seg_q(snr[p]);
        ++ar;
        pk = max(pk, __float_as_uint(snr[p]));
      }
    const long long s0 = seg_sum64(sq, S);
    const int area = seg_sumi(ar, S);
    const float peak = __uint_as_float(seg_maxu(pk, S));
    const float th = S.nd_thresh[x];
    const int nt = S.nd_nthresh[x];
    const double cont = S.nd_cont[x];
    const long long qt = seg_q(th);
    const long long total = s0 - (long long)area * qt;
    if (!(peak > th) || total <= 0) continue;
    float r = peak / th;
    for (int h = nt; h > 1; h >>= 1) r = sqrtf(r);
    float lev = th;
    for (int level = 1; level < nt; ++level) {
      lev = lev * r;
      const int kk = seg_islands((unsigned)x, lev, snr, L, lab, acc, n, S);
      if (S.status != 0) break;
      if (kk < 2) continue;
      const int made = seg_make_children(x, lev, qt, total, cont, nt, A, snr, L, lab, acc, S);
      if (made > 0 || S.status != 0) break;
    }
  }

  // ---- leaves in depth-first order; the pixels a split left over, bottom-up ----
  if (S.status == 0 && S.nnodes > 0) {
    if (tid == 0) {
      const int nn = S.nnodes;
      int stack[kSegNodeCap], sp = 0, nleaf = 0;
      for (int x = nn - 1; x >= 0; --x)
        if (S.nd_parent[x] < 0) stack[sp++] = x;
      while (sp > 0) {
        const int x = stack[--sp];
        if (S.nd_nchild[x] == 0) {
          S.nd_rank[x] = nleaf;
          if (nleaf < kSegObjCap) S.leaf_node[nleaf] = x;
          ++nleaf;
        } else {
          S.nd_rank[x] = -1;
          for (int c = S.nd_nchild[x] - 1; c >= 0; --c) stack[sp++] = S.nd_first[x] + c;
        }
      }
      for (int x = 0; x < nn; ++x) {
        S.nd_lo[x] = S.nd_nchild[x] == 0 ? S.nd_rank[x] : INT_MAX;
        S.nd_hi[x] = S.nd_nchild[x] == 0 ? S.nd_rank[x] : -1;
      }
      for (int x = nn - 1; x >= 0; --x) {
        const int par = S.nd_parent[x];
        if (par >= 0) {
          S.nd_lo[par] = min(S.nd_lo[par], S.nd_lo[x]);
          S.nd_hi[par] = max(S.nd_hi[par], S.nd_hi[x]);
        }
      }
      S.nleaf = nleaf;
      if (nleaf > kSegObjCap) S.status = 1;
    }
    __syncthreads();
  }
  if (S.status == 0 && S.nnodes > 0) {
    for (int x = S.nnodes - 1; x >= 0; --x) {
      if (S.nd_nchild[x] == 0) continue;
      const int lo = S.nd_lo[x], hi = S.nd_hi[x];
      if (tid <= hi - lo) {
        S.lf_key[lo + tid] = 0;
        S.lf_area[lo + tid] = 0;
      }
      __syncthreads();
      for (int p = tid; p < np; p += kSegThreads) {
        const unsigned node = L[p];
        if (node == kSegNoNode || S.nd_nchild[node] != 0) continue;
        const int rk = S.nd_rank[node];
        if (rk < lo || rk > hi) continue;
        atomicAdd(&S.lf_area[rk], 1);
        // the largest snr, its first raster position
        atomicMax(&S.lf_key[rk], ((unsigned long long)__float_as_uint(snr[p]) << 32) | (0xFFFFFFFFu - (unsigned)p));
      }
      __syncthreads();
      if (tid <= hi - lo) {
        const int rk = lo + tid;
        const double size = fmax(sqrt((double)S.lf_area[rk] / M_PI), 1.0);
        S.lf_s2[rk] = size * size;
        const int p = (int)(0xFFFFFFFFu - (unsigned)(S.lf_key[rk] & 0xFFFFFFFFull));
        S.lf_py[rk] = p / n;
        S.lf_px[rk] = p % n;
      }
      __syncthreads();
      for (int p = tid; p < np; p += kSegThreads) {
        if (L[p] != x) continue;
        const int i = p / n, j = p - i * n;
        int best = lo;
        double bestd = 0.0;
        for (int rk = lo; rk <= hi; ++rk) {
          const int dy = i - S.lf_py[rk], dx = j - S.lf_px[rk];
          const double d2 = (double)(dy * dy + dx * dx) / S.lf_s2[rk];
          if (rk == lo || d2 < bestd) {
            bestd = d2;
            best = rk;
          }
        }
        L[p] = (uint8_t)S.leaf_node[best];
      }
      __syncthreads();
    }
  }

  // ---- per-object sums, shapes, clean, the central object ----
  const bool have = S.status == 0 && S.nleaf > 0;
  if (have) {
    const int nleaf = S.nleaf;
    if (tid < nleaf) {
      for (int c = 0; c < 6; ++c) S.ob_sum[tid][c] = 0;
      S.ob_npix[tid] = 0;
      S.ob_kth[tid] = 0;
      S.target[tid] = -1;
    }
    __syncthreads();
    for (int p = tid; p < np; p += kSegThreads) {
      const unsigned node = L[p];
      unsigned rk = kSegNone;
      if (node != kSegNoNode) {
        rk = (unsigned)S.nd_rank[node];
        const int i = p / n, j = p - i * n;
        const long long q = seg_q(snr[p]);
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
          if (rk == kSegNone) continue;
          if (__float_as_uint(snr[p]) >= (S.ob_kth[rk] | (1u << bit))) atomicAdd(&S.ob_cnt[rk], 1);
        }
        __syncthreads();
        if (tid < nleaf && S.ob_cnt[tid] >= A.minarea) S.ob_kth[tid] |= 1u << bit;
        __syncthreads();
      }
      if (tid < nleaf) {
        const double t = (double)S.ob_sum[tid][0];
        const double mx = (double)S.ob_sum[tid][1] / t, my = (double)S.ob_sum[tid][2] / t;
        const double x2 = fmax((double)S.ob_sum[tid][3] / t - mx * mx, 1.0 / 12.0);
        const double y2 = fmax((double)S.ob_sum[tid][4] / t - my * my, 1.0 / 12.0);
        double xy = (double)S.ob_sum[tid][5] / t - mx * my;
        double det = x2 * y2 - xy * xy;
        if (det < 1.0 / 144.0) {
          xy = 0.0;
          det = x2 * y2;
        }
        const double half = 0.5 * (x2 + y2), dif = x2 - y2;
        const double root = sqrt(fmax(0.25 * (dif * dif) + xy * xy, 0.0));
        const double a = sqrt(half + root), b = sqrt(fmax(half - root, 1.0 / 12.0));
        double mth = 0.0;
        if (S.ob_npix[tid] >= A.minarea) mth = fmax((double)__uint_as_float(S.ob_kth[tid]) - (double)th0, 0.0);
        const double unit = M_PI * a * b;
        const double tot = t * (1.0 / kSegFix);
        S.sh_mx[tid] = mx;
        S.sh_my[tid] = my;
        S.sh_a[tid] = a;
        S.sh_cxx[tid] = y2 / det;
        S.sh_cyy[tid] = x2 / det;
        S.sh_cxy[tid] = -2.0 * xy / det;
        S.sh_unit[tid] = unit;
        S.sh_amp[tid] = tot / (2.0 * unit);
        S.sh_mth[tid] = mth;
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
            const double dx = S.sh_mx[i] - S.sh_mx[j], dy = S.sh_my[i] - S.sh_my[j];
            const double zone = 10.0 * (S.sh_a[i] + S.sh_a[j]);
            if (dx * dx + dy * dy >= zone * zone) continue;
            const double ratio = S.sh_amp[j] / thd;
            if (ratio <= 1.0) continue;
            const double alpha = (ratio - 1.0) * S.sh_unit[j] / (double)S.ob_npix[j];
            const double val = 1.0 + alpha * (S.sh_cxx[j] * dx * dx + S.sh_cyy[j] * dy * dy + S.sh_cxy[j] * dx * dy);
            const double wing = (1.0 < val && val < 1e10) ? S.sh_amp[j] / val : 0.0;
            if (wing > S.sh_mth[i] && wing > best) {
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
  const bool fine = S.status == 0;
  const int nobj = fine ? S.nobj : 0, central = S.central;
  for (int p = tid; p < np; p += kSegThreads) {
    int seg = 0;
    if (have && fine && lab[p] != kSegNone) {
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
    if (A.status) A.status[k] = S.status;
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
