// De-blending and cleaning of the objects of whole frames: sep.extract with its defaults deblend_cont = 0.005 and
// clean = True, as the reference calls it (lightcurver/processes/star_extraction.py:23-26), frozen as the SPEC of
// DESIGN.md §5 "De-blending and cleaning of frame objects" and restated in NumPy by tests/_deblend.py.  It is a rewrite
// of the label and count planes of extract.hip between runs of that file's own numbering, box and measure launches:
//   (extract.hip)         labels, then the parents numbered and their boxes made in a table sized by their count;
//   db_deblend_kernel     (twice: boxes of up to 1024 pixels, then the larger ones, each with the LDS its boxes need)
//                         one workgroup per parent with a box of at most 64 x 64: the box of snr and labels into LDS, the
//                         tree walk of segment_kernel (segment.hip) on it, every leaf written back under the raster index
//                         of its own first pixel with count[label] = its pixels; NODEBLEND recorded at the first pixel;
//   (extract.hip)         numbered with minarea 1 (a component below minarea has count 0 and stays no object), boxes,
//                         segmap, mask and the measurement, in a table sized by the count;
//   db_shape_kernel       one workgroup per object: the six integer sums of the measurement again, the minarea-th
//                         largest snr by bisection on the float bits, the shape that clean compares;
//   db_target_kernel      one thread per object i over all j of its frame, float64;
//   db_resolve_kernel     every object follows its targets to the survivor, which collects the smallest label and the
//                         pixel count of its union by integer atomics;
//   db_relabel_kernel, db_recount_kernel
//                         the pixels take the union's label, count[label] its pixels; then (extract.hip) a third time;
//   db_finish_kernel      the first max_objects rows into the caller's table with the NODEBLEND bit, nobj and status 1.
// As in extract.hip no workgroup waits for another within a launch; every loop over labels or targets is bounded and
// the bound sets status 2.  The tree walk is still a copy, of deblend_tree.h's device functions (segment_kernel's) without
// the groups of a stamp: instantiated from that header this kernel measured 4 to 6 % slower for a reason that was not
// found (DESIGN.md gives the figures), so the copy stays until it is.  The shape and the wing of clean are clean_shape.h,
// shared with segment_kernel.  Offsets into the planes are 64-bit.
#pragma clang fp contract(off)  // the SPEC fixes every rounding: no fused multiply-adds, on the device or the host

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "block_reduce.h"
#include "clean_shape.h"
#include "device_call.h"
#include "frame_steps.h"
#include "lc_common.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kDbThreads = 256;
constexpr int kDbWaves = kDbThreads / 64;
constexpr int kDbBox = 64;                     // the longest side of a box that is de-blended
constexpr int kDbPixels = kDbBox * kDbBox;
constexpr int kDbLeafCap = LC_SEGMENT_MAX_OBJECTS;  // leaves of one parent's tree
constexpr int kDbNodeCap = 64;                 // nodes of that tree, the parent included
constexpr unsigned kDbNone = 0xFFFFu;
constexpr unsigned kDbNoNode = 0xFFu;
constexpr double kDbFix = 1048576.0;           // 2^20: the tree's deciding sums
constexpr double kDbMomentFix = 1024.0;        // 2^10: the measurement's sums, which the shapes of clean take
constexpr float kDbSnrLimit = 65536.0f;
constexpr int kDbLargeBox = 512;
constexpr int kDbAux = 6;                      // first, npix, xmin, xmax, ymin, ymax: a row of extract.hip's table
constexpr int kDbGrid = 4096;
constexpr int kDbSmallPixels = 1024;           // boxes up to here go to a launch with a quarter of the LDS
constexpr size_t kDbLdsPerPixel = 15;          // acc 8, snr 4, lab 2, node 1 bytes

typedef unsigned long long u64;

struct DbShared {
  long long red64[kDbWaves];
  int redi[kDbWaves];
  unsigned redu[kDbWaves];
  double nd_cont[kDbNodeCap];
  float nd_thresh[kDbNodeCap];
  int nd_nthresh[kDbNodeCap], nd_first[kDbNodeCap], nd_nchild[kDbNodeCap], nd_parent[kDbNodeCap];
  int nd_rank[kDbNodeCap], nd_lo[kDbNodeCap], nd_hi[kDbNodeCap];
  int list[kDbNodeCap];
  int nnodes, status, ngood, nleaf;
  int leaf_node[kDbLeafCap];
  u64 lf_key[kDbLeafCap];
  int lf_area[kDbLeafCap], lf_py[kDbLeafCap], lf_px[kDbLeafCap];
  double lf_s2[kDbLeafCap];
  int lf_first[kDbLeafCap], lf_npix[kDbLeafCap];
};

__device__ __forceinline__ long long db_q(float v) { return (long long)rint((double)v * kDbFix); }

__device__ __forceinline__ long long db_sum64(long long v, DbShared &S) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) S.red64[threadIdx.x >> 6] = v;
  __syncthreads();
  long long r = 0;
  for (int w = 0; w < kDbWaves; ++w) r += S.red64[w];
  __syncthreads();
  return r;
}

__device__ __forceinline__ int db_sumi(int v, DbShared &S) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) S.redi[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
  for (int w = 0; w < kDbWaves; ++w) r += S.redi[w];
  __syncthreads();
  return r;
}

__device__ __forceinline__ unsigned db_maxu(unsigned v, DbShared &S) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_down((int)v, o, 64));
  if ((threadIdx.x & 63) == 0) S.redu[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned r = 0;
  for (int w = 0; w < kDbWaves; ++w) r = max(r, S.redu[w]);
  __syncthreads();
  return r;
}

// 8-connected islands of {p : L[p] == node and snr[p] > lev} in the bw x bh box: lab[p] = the island's first pixel in
// raster order (kDbNone outside the set).  Returns the number of islands (0 or 1 without labelling below two pixels).
__device__ int db_islands(unsigned node, float lev, const float *snr, const uint8_t *L, uint16_t *lab, long long *acc,
                          int bw, int bh, DbShared &S) {
  const int np = bw * bh, tid = threadIdx.x;
  int cnt = 0;
  for (int p = tid; p < np; p += kDbThreads) {
    const bool m = L[p] == node && snr[p] > lev;
    lab[p] = m ? (uint16_t)p : (uint16_t)kDbNone;
    cnt += m;
  }
  const int members = db_sumi(cnt, S);
  if (members == 0) return 0;
  bool converged = members == 1;
  for (int sweep = 0; sweep < np && !converged; ++sweep) {
    int changed = 0;
    for (int p = tid; p < np; p += kDbThreads) {
      const unsigned l = lab[p];
      if (l == kDbNone) continue;
      const int i = p / bw, j = p - i * bw;
      unsigned m = l;
      for (int y = max(i - 1, 0); y <= min(i + 1, bh - 1); ++y)
        for (int x = max(j - 1, 0); x <= min(j + 1, bw - 1); ++x) m = min(m, (unsigned)lab[y * bw + x]);
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
  for (int p = tid; p < np; p += kDbThreads)
    if (lab[p] == p) {
      acc[p] = 0;
      ++cnt;
    }
  return db_sumi(cnt, S);
}

// The islands labelled in lab become child nodes of `parent` where their flux is at least cont * total; a split needs two
// of them.  Returns the number of children made (0: nothing changed).  Sets status 1 when the work list is full.
__device__ int db_make_children(int parent, float lev, long long qt, long long total, double cont, int nthresh, int np,
                                const float *snr, uint8_t *L, const uint16_t *lab, long long *acc, DbShared &S) {
  const int tid = threadIdx.x;
  if (tid == 0) S.ngood = 0;
  for (int p = tid; p < np; p += kDbThreads) {
    const unsigned l = lab[p];
    if (l == kDbNone) continue;
    atomicAdd((u64 *)&acc[l], (u64)(db_q(snr[p]) - qt));
  }
  __syncthreads();
  const double bar = cont * (double)total;
  for (int p = tid; p < np; p += kDbThreads) {
    if (lab[p] != p) continue;
    const bool good = (double)acc[p] >= bar;
    int slot = kDbNodeCap;
    if (good) slot = atomicAdd(&S.ngood, 1);
    if (slot < kDbNodeCap)
      S.list[slot] = p;
    else
      acc[p] = -1;
  }
  __syncthreads();
  const int ngood = S.ngood, base = S.nnodes;
  if (ngood < 2) return 0;
  if (base + ngood > kDbNodeCap) {
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
    S.nd_nthresh[id] = max(nthresh / 2, 4);
    S.nd_cont[id] = f > 0 ? bar / (double)f : 0.0;
    S.nd_first[id] = 0;
    S.nd_nchild[id] = 0;
    S.nd_parent[id] = parent;
    acc[p] = id;
  }
  __syncthreads();
  for (int p = tid; p < np; p += kDbThreads) {
    const unsigned l = lab[p];
    if (l == kDbNone) continue;
    const long long c = acc[l];
    if (c >= 0) L[p] = (uint8_t)c;
  }
  if (tid == 0) {
    S.nd_first[parent] = base;
    S.nd_nchild[parent] = ngood;
    S.nnodes = base + ngood;
  }
  __syncthreads();
  return ngood;
}

struct DbDeblendArgs {
  int K, h, w, cap;  // cap: rows of the parents' table per frame
  int above, upto;   // this launch takes the boxes of above < pixels <= upto, which is what its LDS planes hold
  int nthresh;
  float thresh;
  double cont;
  const float *snr;
  const int32_t *paux, *pnobj;
  int32_t *label, *count, *status;
  uint8_t *nodeblend;
};

__global__ __launch_bounds__(kDbThreads) void db_deblend_kernel(DbDeblendArgs A) {
  extern __shared__ __align__(16) unsigned char db_lds[];
  __shared__ DbShared S;
  long long *acc = (long long *)db_lds;
  float *snr = (float *)(acc + A.upto);
  uint16_t *lab = (uint16_t *)(snr + A.upto);
  uint8_t *L = (uint8_t *)(lab + A.upto);
  const int tid = threadIdx.x;
  const size_t hw = (size_t)A.h * A.w;
  const long long slots = (long long)A.K * A.cap;
  for (long long s = blockIdx.x; s < slots; s += gridDim.x) {
    const int frame = (int)(s / A.cap), i = (int)(s - (long long)frame * A.cap);
    if (i >= min(A.pnobj[frame], A.cap)) continue;  // the same for every lane
    const int32_t *a = A.paux + (size_t)s * kDbAux;
    const int first = a[0], npix = a[1], xmin = a[2], xmax = a[3], ymin = a[4], ymax = a[5];
    if (xmin < 0 || ymin < 0 || xmax >= A.w || ymax >= A.h || xmin > xmax || ymin > ymax) continue;  // no box was made
    const size_t base = (size_t)frame * hw;
    const int bw = xmax - xmin + 1, bh = ymax - ymin + 1;
    if (bw > kDbBox || bh > kDbBox) {  // kept whole: said by the launch of the small boxes
      if (tid == 0 && A.above == 0) {
        A.count[base + first] = npix;
        A.nodeblend[base + first] = 1;
      }
      continue;
    }
    const int np = bw * bh;
    if (np <= A.above || np > A.upto) continue;  // the other launch's
    __syncthreads();  // the planes and S of the parent before
    int bad = 0;
    for (int p = tid; p < np; p += kDbThreads) {
      const int y = p / bw, x = p - y * bw;
      const size_t g = base + (size_t)(ymin + y) * A.w + (xmin + x);
      const bool mine = A.label[g] == first;
      const float v = A.snr[g];
      snr[p] = v;
      L[p] = mine ? (uint8_t)0 : (uint8_t)kDbNoNode;
      bad |= (mine && !(v < kDbSnrLimit)) ? 1 : 0;
    }
    if (tid == 0) {
      S.status = 0;
      S.nnodes = 1;
      S.nleaf = 0;
      S.nd_thresh[0] = A.thresh;
      S.nd_nthresh[0] = A.nthresh;
      S.nd_cont[0] = A.cont;
      S.nd_first[0] = 0;
      S.nd_nchild[0] = 0;
      S.nd_parent[0] = -1;
    }
    if (__syncthreads_or(bad)) {  // flagged RANGE by the measurement: kept whole, without the bit
      if (tid == 0) A.count[base + first] = npix;
      continue;
    }

    // ---- the work list of the tree, in creation order ----
    for (int x = 0; S.status == 0 && x < S.nnodes; ++x) {
      long long sq = 0;
      int ar = 0;
      unsigned pk = 0;
      for (int p = tid; p < np; p += kDbThreads)
        if (L[p] == x) {
          sq += db_q(snr[p]);
          ++ar;
          pk = max(pk, __float_as_uint(snr[p]));
        }
      const long long s0 = db_sum64(sq, S);
      const int area = db_sumi(ar, S);
      const float peak = __uint_as_float(db_maxu(pk, S));
      const float th = S.nd_thresh[x];
      const int nt = S.nd_nthresh[x];
      const double cont = S.nd_cont[x];
      const long long qt = db_q(th);
      const long long total = s0 - (long long)area * qt;
      if (!(peak > th) || total <= 0) continue;
      float r = peak / th;
      for (int hh = nt; hh > 1; hh >>= 1) r = sqrtf(r);
      float lev = th;
      for (int level = 1; level < nt; ++level) {
        lev = lev * r;
        const int kk = db_islands((unsigned)x, lev, snr, L, lab, acc, bw, bh, S);
        if (S.status != 0) break;
        if (kk < 2) continue;
        const int made = db_make_children(x, lev, qt, total, cont, nt, np, snr, L, lab, acc, S);
        if (made > 0 || S.status != 0) break;
      }
    }

    // ---- leaves in depth-first order; the pixels a split left over, from the last node to the first ----
    if (S.status == 0 && S.nnodes > 1) {
      if (tid == 0) {
        const int nn = S.nnodes;
        int *stack = S.list, sp = 0, nleaf = 0;  // (the list of db_make_children is free by now)
        stack[sp++] = 0;
        while (sp > 0) {
          const int x = stack[--sp];
          if (S.nd_nchild[x] == 0) {
            S.nd_rank[x] = nleaf;
            if (nleaf < kDbLeafCap) S.leaf_node[nleaf] = x;
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
        if (nleaf > kDbLeafCap) S.status = 1;
      }
      __syncthreads();
    }
    if (S.status == 0 && S.nnodes > 1) {
      for (int x = S.nnodes - 1; x >= 0; --x) {
        if (S.nd_nchild[x] == 0) continue;
        const int lo = S.nd_lo[x], hi = S.nd_hi[x];
        if (tid <= hi - lo) {
          S.lf_key[lo + tid] = 0;
          S.lf_area[lo + tid] = 0;
        }
        __syncthreads();
        for (int p = tid; p < np; p += kDbThreads) {
          const unsigned node = L[p];
          if (node == kDbNoNode || S.nd_nchild[node] != 0) continue;
          const int rk = S.nd_rank[node];
          if (rk < lo || rk > hi) continue;
          atomicAdd(&S.lf_area[rk], 1);
          // the largest snr, its first raster position
          atomicMax(&S.lf_key[rk], ((u64)__float_as_uint(snr[p]) << 32) | (0xFFFFFFFFu - (unsigned)p));
        }
        __syncthreads();
        if (tid <= hi - lo) {
          const int rk = lo + tid;
          const double size = fmax(sqrt((double)S.lf_area[rk] / M_PI), 1.0);
          S.lf_s2[rk] = size * size;
          const int p = (int)(0xFFFFFFFFu - (unsigned)(S.lf_key[rk] & 0xFFFFFFFFull));
          S.lf_py[rk] = p / bw;
          S.lf_px[rk] = p % bw;
        }
        __syncthreads();
        for (int p = tid; p < np; p += kDbThreads) {
          if (L[p] != x) continue;
          const int i2 = p / bw, j2 = p - i2 * bw;
          int best = lo;
          double bestd = 0.0;
          for (int rk = lo; rk <= hi; ++rk) {
            const int dy = i2 - S.lf_py[rk], dx = j2 - S.lf_px[rk];
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

    // ---- the planes: every leaf under its own first pixel ----
    const int status = S.status;
    if (status == 2) {
      if (tid == 0) atomicMax(A.status + frame, 2);
    } else if (status == 1 || S.nnodes == 1) {  // a capacity: whole, with the bit; no split: as it was
      if (tid == 0) {
        A.count[base + first] = npix;
        if (status == 1) A.nodeblend[base + first] = 1;
      }
    } else {
      const int nleaf = S.nleaf;
      if (tid < nleaf) {
        S.lf_first[tid] = INT_MAX;
        S.lf_npix[tid] = 0;
      }
      __syncthreads();
      for (int p = tid; p < np; p += kDbThreads) {
        const unsigned node = L[p];
        if (node == kDbNoNode) continue;
        const int rk = S.nd_rank[node];
        atomicMin(&S.lf_first[rk], p);  // the raster order of the box is that of the frame
        atomicAdd(&S.lf_npix[rk], 1);
      }
      __syncthreads();
      for (int p = tid; p < np; p += kDbThreads) {
        const unsigned node = L[p];
        if (node == kDbNoNode) continue;
        const int f = S.lf_first[S.nd_rank[node]], fy = f / bw, fx = f - fy * bw;
        const int y = p / bw, x = p - y * bw;
        A.label[base + (size_t)(ymin + y) * A.w + (xmin + x)] = (ymin + fy) * A.w + (xmin + fx);
      }
      if (tid < nleaf) {
        const int f = S.lf_first[tid], fy = f / bw, fx = f - fy * bw;
        A.count[base + (size_t)(ymin + fy) * A.w + (xmin + fx)] = S.lf_npix[tid];
      }
    }
  }
}

// ---- clean ----------------------------------------------------------------------------------------------------------------

struct DbCleanArgs {
  int K, h, w, cap;  // cap: rows of the objects' tables per frame
  int minarea, max_objects;
  float thresh;
  const float *snr;
  const int32_t *faux, *fnobj;
  const lc_extract_object *fobj;
  int32_t *label, *count, *status;
  uint8_t *nodeblend;
  CleanShape *shape;  // valid = 0: no part in clean
  int32_t *target, *root, *minlab, *unpix;
  lc_extract_object *objects;
  int32_t *nobj;
};

__global__ __launch_bounds__(kDbThreads) void db_shape_kernel(DbCleanArgs A) {
  __shared__ u64 s_u[kDbWaves];
  __shared__ int s_i[kDbWaves];
  const int tid = threadIdx.x;
  const size_t hw = (size_t)A.h * A.w;
  const long long slots = (long long)A.K * A.cap;
  for (long long s = blockIdx.x; s < slots; s += gridDim.x) {
    const int frame = (int)(s / A.cap), i = (int)(s - (long long)frame * A.cap);
    const int n = min(A.fnobj[frame], A.cap);
    if (i >= n || n < 2) continue;  // the same for every lane
    const int32_t *a = A.faux + (size_t)s * kDbAux;
    const int first = a[0], npix = a[1], xmin = a[2], xmax = a[3], ymin = a[4], ymax = a[5];
    const bool boxed = !(xmin < 0 || ymin < 0 || xmax >= A.w || ymax >= A.h || xmin > xmax || ymin > ymax);
    if (!boxed || (A.fobj[s].flag & 3)) {  // LARGE or RANGE: no part in clean
      if (tid == 0) {
        CleanShape z;
        memset(&z, 0, sizeof(z));
        A.shape[s] = z;
      }
      continue;
    }
    const size_t base = (size_t)frame * hw;
    const unsigned bw = (unsigned)(xmax - xmin + 1), bh = (unsigned)(ymax - ymin + 1);
    const u64 count = (u64)bw * bh;
    u64 s0 = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    for (u64 j = tid; j < count; j += kDbThreads) {
      const unsigned r = (unsigned)(j / bw), c = (unsigned)(j - (u64)r * bw);
      const size_t g = base + (size_t)(ymin + (int)r) * A.w + (xmin + (int)c);
      if (A.label[g] != first) continue;
      const u64 q = (u64)(long long)rint((double)A.snr[g] * kDbMomentFix);
      const u64 dx = c, dy = r;
      s0 += q;
      sx += q * dx;
      sy += q * dy;
      sxx += q * dx * dx;
      syy += q * dy * dy;
      sxy += q * dx * dy;
    }
    s0 = block_sum<kDbWaves>(s0, s_u);
    sx = block_sum<kDbWaves>(sx, s_u);
    sy = block_sum<kDbWaves>(sy, s_u);
    sxx = block_sum<kDbWaves>(sxx, s_u);
    syy = block_sum<kDbWaves>(syy, s_u);
    sxy = block_sum<kDbWaves>(sxy, s_u);
    // the minarea-th largest snr: its bits, built from the top bit down (a detected snr is positive)
    unsigned kth = 0;
    if (npix >= A.minarea) {
      for (int bit = 30; bit >= 0; --bit) {
        const unsigned cand = kth | (1u << bit);
        int cnt = 0;
        for (u64 j = tid; j < count; j += kDbThreads) {
          const unsigned r = (unsigned)(j / bw), c = (unsigned)(j - (u64)r * bw);
          const size_t g = base + (size_t)(ymin + (int)r) * A.w + (xmin + (int)c);
          if (A.label[g] == first && __float_as_uint(A.snr[g]) >= cand) ++cnt;
        }
        if (block_sum<kDbWaves>(cnt, s_i) >= A.minarea) kth = cand;
      }
    }
    if (tid == 0) {
      CleanShape z;
      memset(&z, 0, sizeof(z));
      if (s0 > 0)
        z = clean_shape((double)s0, (double)sx, (double)sy, (double)sxx, (double)syy, (double)sxy, kDbMomentFix, npix,
                        A.minarea, kth, A.thresh, (double)xmin, (double)ymin);
      A.shape[s] = z;
    }
  }
}

// the target of every object on its own: the brighter object whose wing at i's centre is the largest above i's mthresh
__global__ __launch_bounds__(kDbThreads) void db_target_kernel(DbCleanArgs A) {
  const long long s = (long long)blockIdx.x * kDbThreads + threadIdx.x;
  if (s >= (long long)A.K * A.cap) return;
  const int frame = (int)(s / A.cap), i = (int)(s - (long long)frame * A.cap);
  const int n = min(A.fnobj[frame], A.cap);
  if (i >= n) return;
  A.minlab[s] = INT_MAX;
  A.unpix[s] = 0;
  int into = -1;
  if (n >= 2) {
    const CleanShape *sh = A.shape + (size_t)frame * A.cap;
    const CleanShape me = sh[i];
    if (me.valid) {
      const double thd = (double)A.thresh;
      double best = 0.0;
      for (int j = 0; j < n; ++j) {
        const CleanShape o = sh[j];
        if (j == i || !o.valid || o.s0 <= me.s0) continue;
        const double wing = clean_wing(me, o, thd);
        if (wing > me.mth && wing > best) {
          best = wing;
          into = j;
        }
      }
    }
  }
  A.target[s] = into;
}

// along a chain the sum of q rises strictly, so it ends within n steps
__global__ __launch_bounds__(kDbThreads) void db_resolve_kernel(DbCleanArgs A) {
  const long long s = (long long)blockIdx.x * kDbThreads + threadIdx.x;
  if (s >= (long long)A.K * A.cap) return;
  const int frame = (int)(s / A.cap), i = (int)(s - (long long)frame * A.cap);
  const int n = min(A.fnobj[frame], A.cap);
  if (i >= n) return;
  const size_t row = (size_t)frame * A.cap;
  int r = i, steps = 0;
  for (; steps <= n; ++steps) {
    const int t = A.target[row + r];
    if (t < 0 || t >= n) break;
    r = t;
  }
  if (steps > n) {
    atomicMax(A.status + frame, 2);
    r = i;
  }
  A.root[s] = r;
  const int32_t *a = A.faux + (size_t)s * kDbAux;
  atomicMin(A.minlab + row + r, a[0]);
  atomicAdd(A.unpix + row + r, a[1]);
}

__global__ __launch_bounds__(kDbThreads) void db_relabel_kernel(DbCleanArgs A) {
  const size_t hw = (size_t)A.h * A.w;
  for (size_t frame = blockIdx.y; frame < (size_t)A.K; frame += gridDim.y) {
    const int n = min(A.fnobj[frame], A.cap);
    const size_t base = frame * hw, row = frame * (size_t)A.cap;
    for (size_t p = (size_t)blockIdx.x * kDbThreads + threadIdx.x; p < hw; p += (size_t)gridDim.x * kDbThreads) {
      const int l = A.label[base + p];
      if (l < 0) continue;
      const int num = A.count[base + l];  // the object number: not written in this launch
      if (num < 1 || num > n) continue;
      const int nl = A.minlab[row + A.root[row + num - 1]];
      if (nl != l) A.label[base + p] = nl;
    }
  }
}

// count[label] = the pixels of the union at the label it now has, 0 at the labels it gave up; the bit goes along
__global__ __launch_bounds__(kDbThreads) void db_recount_kernel(DbCleanArgs A) {
  const long long s = (long long)blockIdx.x * kDbThreads + threadIdx.x;
  if (s >= (long long)A.K * A.cap) return;
  const int frame = (int)(s / A.cap), i = (int)(s - (long long)frame * A.cap);
  const int n = min(A.fnobj[frame], A.cap);
  if (i >= n) return;
  const size_t row = (size_t)frame * A.cap, base = (size_t)frame * A.h * A.w;
  const int first = A.faux[(size_t)s * kDbAux], r = A.root[s], nl = A.minlab[row + r];
  A.count[base + first] = first == nl ? A.unpix[row + r] : 0;
  if (first != nl && A.nodeblend[base + first]) A.nodeblend[base + nl] = 1;
}

__global__ __launch_bounds__(kDbThreads) void db_finish_kernel(DbCleanArgs A) {
  const long long s = (long long)blockIdx.x * kDbThreads + threadIdx.x;
  if (s >= (long long)A.K * A.cap) return;
  const int frame = (int)(s / A.cap), i = (int)(s - (long long)frame * A.cap);
  const int n = min(A.fnobj[frame], A.cap);
  if (i == 0) {
    A.nobj[frame] = n;
    if (n > A.max_objects && A.status[frame] == 0) A.status[frame] = 1;
  }
  if (i >= n || i >= A.max_objects || !A.objects) return;
  // the row as six 16-byte words (rows are 96 bytes in buffers of their own); flag is the first int of the third
  const uint4 *src = (const uint4 *)(A.fobj + s);
  uint4 *dst = (uint4 *)(A.objects + (size_t)frame * A.max_objects + i);
  const unsigned bit = A.nodeblend[(size_t)frame * A.h * A.w + A.fobj[s].first] ? LC_EXTRACT_FLAG_NODEBLEND : 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    uint4 v = src[k];
    if (k == 2) v.x |= bit;
    dst[k] = v;
  }
}
static_assert(sizeof(lc_extract_object) == 96 && offsetof(lc_extract_object, flag) == 32, "db_finish_kernel copies by words");

// ---- host -------------------------------------------------------------------------------------------------------------------

const char *deblend_cfg_error(const lc_deblend_cfg *d, int *code) {
  *code = LC_ERR_INVALID;
  if (!d) return "a missing de-blending configuration";
  if (!std::isfinite(d->deblend_cont) || !(d->deblend_cont >= 0.0f)) return "deblend_cont must be finite and >= 0";
  *code = LC_ERR_UNSUPPORTED;
  if (d->clean_param != 1.0f) return "only clean_param = 1 is built";
  const int nt = d->deblend_nthresh;
  if (nt != 4 && nt != 8 && nt != 16 && nt != 32) return "deblend_nthresh must be 4, 8, 16 or 32";
  return nullptr;
}

// the largest of K counts on the device, after the launches before it
static hipError_t db_largest(lc_ctx *ctx, int K, const int32_t *d, int *largest) {
  std::vector<int32_t> host((size_t)K);
  hipError_t e = hipMemcpyAsync(host.data(), d, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  *largest = 0;
  for (int32_t v : host) *largest = std::max(*largest, (int)v);
  return e;
}

static unsigned db_blocks(long long slots) { return (unsigned)((slots + kDbThreads - 1) / kDbThreads); }

hipError_t deblend_launch(lc_ctx *ctx, DeviceCall &call, int K, int h, int w, const lc_extract_cfg *cfg,
                          const lc_deblend_cfg *dcfg, int max_objects, const ExtractBuffers &B) {
  hipStream_t st = ctx->stream;
  const size_t hw = (size_t)h * w, tot = (size_t)K * hw;
  const int64_t rows_limit = ((int64_t)1 << 31) / kDbAux;
  hipError_t e = hipSuccess;
  if (B.objects) e = hipMemsetAsync(B.objects, 0, (size_t)K * max_objects * sizeof(lc_extract_object), st);
  if (e != hipSuccess) return e;

  // ---- the parents ----
  ExtractBuffers P = B;
  P.objects = nullptr;
  P.segmap = nullptr;
  P.mask = nullptr;
  P.aux = nullptr;
  uint8_t *nodeblend = nullptr;
  if ((e = call.alloc((size_t)K, &P.nobj)) != hipSuccess) return e;
  if ((e = call.alloc(tot, &nodeblend)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(nodeblend, 0, tot, st)) != hipSuccess) return e;
  if ((e = extract_label_launch(ctx, K, h, w, cfg, P)) != hipSuccess) return e;
  if ((e = extract_count_launch(ctx, K, h, w, cfg->minarea, INT_MAX, P)) != hipSuccess) return e;
  int pcap = 0;
  if ((e = db_largest(ctx, K, P.nobj, &pcap)) != hipSuccess) return e;
  pcap = std::max(pcap, 1);
  if ((int64_t)K * pcap >= rows_limit) return hipErrorInvalidValue;
  if ((e = call.alloc((size_t)K * pcap * kDbAux, &P.aux)) != hipSuccess) return e;
  if ((e = extract_table_launch(ctx, K, h, w, cfg->minarea, pcap, P)) != hipSuccess) return e;

  DbDeblendArgs D;
  D.K = K;
  D.h = h;
  D.w = w;
  D.cap = pcap;
  D.nthresh = dcfg->deblend_nthresh;
  D.thresh = cfg->thresh;
  D.cont = (double)dcfg->deblend_cont;
  D.snr = B.snr;
  D.paux = P.aux;
  D.pnobj = P.nobj;
  D.label = B.label;
  D.count = B.count;
  D.status = B.status;
  D.nodeblend = nodeblend;
  if ((e = hipFuncSetAttribute((const void *)db_deblend_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(kDbPixels * kDbLdsPerPixel))) != hipSuccess)
    return e;
  // twice: the boxes of up to 1024 pixels (most stars) with 15 KiB of planes, so that eight workgroups share a CU, then
  // the larger ones with 60 KiB; a parent is taken by the one launch whose range holds its box
  for (int pass = 0; pass < 2; ++pass) {
    D.above = pass == 0 ? 0 : kDbSmallPixels;
    D.upto = pass == 0 ? kDbSmallPixels : kDbPixels;
    hipLaunchKernelGGL(db_deblend_kernel, dim3((unsigned)std::min<long long>((long long)K * pcap, kDbGrid)),
                       dim3(kDbThreads), (size_t)D.upto * kDbLdsPerPixel, st, D);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }

  // ---- the objects: the parents kept whole and the leaves, whatever their size ----
  ExtractBuffers F = B;
  F.objects = nullptr;
  F.aux = nullptr;
  if ((e = call.alloc((size_t)K, &F.nobj)) != hipSuccess) return e;
  if ((e = extract_count_launch(ctx, K, h, w, 1, INT_MAX, F)) != hipSuccess) return e;
  int fcap = 0;
  if ((e = db_largest(ctx, K, F.nobj, &fcap)) != hipSuccess) return e;
  const bool clean = dcfg->clean != 0 && fcap >= 2;
  fcap = std::max(fcap, 1);
  if ((int64_t)K * fcap >= rows_limit) return hipErrorInvalidValue;
  const size_t rows = (size_t)K * fcap;
  if ((e = call.alloc(rows * kDbAux, &F.aux)) != hipSuccess) return e;
  if ((e = call.alloc(rows, &F.objects)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(F.objects, 0, rows * sizeof(lc_extract_object), st)) != hipSuccess) return e;
  if ((e = extract_table_launch(ctx, K, h, w, 1, fcap, F)) != hipSuccess) return e;

  DbCleanArgs C;
  memset(&C, 0, sizeof(C));
  C.K = K;
  C.h = h;
  C.w = w;
  C.cap = fcap;
  C.minarea = cfg->minarea;
  C.max_objects = max_objects;
  C.thresh = cfg->thresh;
  C.snr = B.snr;
  C.faux = F.aux;
  C.fnobj = F.nobj;
  C.fobj = F.objects;
  C.label = B.label;
  C.count = B.count;
  C.status = B.status;
  C.nodeblend = nodeblend;
  C.objects = B.objects;
  C.nobj = B.nobj;
  if (clean) {
    if ((e = call.alloc(rows, &C.shape)) != hipSuccess) return e;
    if ((e = call.alloc(rows, &C.target)) != hipSuccess) return e;
    if ((e = call.alloc(rows, &C.root)) != hipSuccess) return e;
    if ((e = call.alloc(rows, &C.minlab)) != hipSuccess) return e;
    if ((e = call.alloc(rows, &C.unpix)) != hipSuccess) return e;
    const unsigned per_object = db_blocks((long long)rows);
    hipLaunchKernelGGL(db_shape_kernel, dim3((unsigned)std::min<long long>((long long)rows, kDbGrid)), dim3(kDbThreads), 0, st,
                       C);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(db_target_kernel, dim3(per_object), dim3(kDbThreads), 0, st, C);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(db_resolve_kernel, dim3(per_object), dim3(kDbThreads), 0, st, C);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(db_relabel_kernel,
                       dim3((unsigned)std::min<size_t>((hw + kDbThreads - 1) / kDbThreads, 4096), (unsigned)std::min(K, 65535)),
                       dim3(kDbThreads), 0, st, C);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(db_recount_kernel, dim3(per_object), dim3(kDbThreads), 0, st, C);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the survivors: fewer objects than before, so the same tables hold them
    if ((e = extract_count_launch(ctx, K, h, w, 1, INT_MAX, F)) != hipSuccess) return e;
    if ((e = extract_table_launch(ctx, K, h, w, 1, fcap, F)) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(db_finish_kernel, dim3(db_blocks((long long)rows)), dim3(kDbThreads), 0, st, C);
  return hipGetLastError();
}

}  // namespace lc

using namespace lc;

extern "C" {

int lc_extract_frames_deblended(lc_ctx *ctx, int K, int h, int w, const float *data, const float *var,
                                const float *var_scalar, const lc_extract_cfg *cfg, const lc_deblend_cfg *dcfg,
                                int max_objects, lc_extract_object *objects, int32_t *nobj, int32_t *segmap, uint8_t *mask,
                                int32_t *status, float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  if (K < 1 || h < 1 || w < 1 || !data || (!var && !var_scalar) || !nobj || !status || max_objects < 1)
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_extract_frames_deblended: invalid argument");
  if (const char *why = extract_cfg_error(cfg))
    LC_FAIL(ctx, LC_ERR_INVALID, std::string("lc_extract_frames_deblended: ") + why);
  int code = 0;
  if (const char *why = deblend_cfg_error(dcfg, &code))
    LC_FAIL(ctx, code, std::string("lc_extract_frames_deblended: ") + why);
  if (!lc_extract_supported(h, w) || !extract_batch_fits(K, h, w) ||
      (int64_t)K * max_objects >= ((int64_t)1 << 31) / kDbAux)
    LC_FAIL(ctx, LC_ERR_UNSUPPORTED,
            "lc_extract_frames_deblended: frames of 2^31 pixels or more, or more of them than one grid takes");
  LC_ENTER(ctx);
  const size_t tot = (size_t)K * h * w;
  DeviceCall call(ctx);
  ExtractBuffers B;
  LC_HIP(ctx, call.upload(data, tot, &B.data));
  LC_HIP(ctx, call.upload(var, tot, &B.var));
  if (!var) LC_HIP(ctx, call.upload(var_scalar, (size_t)K, &B.var_scalar));
  LC_HIP(ctx, call.result(objects, (size_t)K * max_objects, &B.objects));
  LC_HIP(ctx, call.result(nobj, (size_t)K, &B.nobj));
  LC_HIP(ctx, call.result(segmap, tot, &B.segmap));
  LC_HIP(ctx, call.result(mask, tot, &B.mask));
  LC_HIP(ctx, call.result(status, (size_t)K, &B.status));
  LC_HIP(ctx, extract_scratch(call, K, h, w, 1, false, &B));
  LC_HIP(ctx, call.start());
  LC_HIP(ctx, deblend_launch(ctx, call, K, h, w, cfg, dcfg, max_objects, B));
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

}  // extern "C"
