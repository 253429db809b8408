// The de-blending tree walk of sep.extract on a bw x bh box held in LDS, in the form that serves both kinds of box: a
// square stamp whose top-level nodes are the groups of the stamp (segment_kernel, segment.hip, which instantiates it) and
// the box of one parent of a frame with a single root (db_deblend_kernel, deblend.hip, which still carries a copy of its
// own: see that file's header).  The SPEC is that of DESIGN.md §5 "Source masking", restated by tests/_segment.py, which
// tests/_deblend.py calls for the frames.  Every sum that decides something is an exact 64-bit integer sum of the 2^-20
// fixed point.  Device only; one workgroup of kTreeThreads walks a box with uniform control flow, and every atomic is
// on LDS.
#pragma once
#pragma clang fp contract(off)  // the SPEC fixes every rounding, whatever the including file sets

#include <climits>
#include <cmath>

#include "block_reduce.h"
#include "lc_common.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kTreeThreads = 256;  // the launch bounds of a kernel that walks a box: it asserts so
constexpr int kTreeWaves = kTreeThreads / kWave;
constexpr int kTreeNodeCap = 64;                      // nodes of the trees of one box, the groups included: the work list
constexpr int kTreeLeafCap = LC_SEGMENT_MAX_OBJECTS;  // leaves of those trees (objects before clean)
constexpr unsigned kTreeNone = 0xFFFFu;               // lab: no island
constexpr unsigned kTreeNoNode = 0xFFu;               // L: no node
constexpr double kTreeFix = 1048576.0;                // 2^20
constexpr float kTreeSnrLimit = 65536.0f;             // fixed-point range of a detected pixel
constexpr size_t kTreeLdsPerPixel = 15;               // acc 8, snr 4, lab 2, L 1 bytes

// the planes of a box, in the order that keeps each aligned: `pixels` of each (at least bw * bh)
struct TreeBox {
  long long *acc;  // a 64-bit accumulator per pixel, indexed by an island's first pixel
  float *snr;
  uint16_t *lab;  // the island of a pixel: its first pixel in raster order
  uint8_t *L;     // the tree node that owns a pixel
  int bw, bh;

  __device__ TreeBox(unsigned char *lds, int pixels, int bw_, int bh_) : bw(bw_), bh(bh_) {
    acc = (long long *)lds;
    snr = (float *)(acc + pixels);
    lab = (uint16_t *)(snr + pixels);
    L = (uint8_t *)(lab + pixels);
  }
};

struct TreeShared {
  long long red64[kTreeWaves];
  int redi[kTreeWaves];
  unsigned redu[kTreeWaves];
  double nd_cont[kTreeNodeCap];
  float nd_thresh[kTreeNodeCap];
  int nd_nthresh[kTreeNodeCap], nd_first[kTreeNodeCap], nd_nchild[kTreeNodeCap], nd_parent[kTreeNodeCap];
  int nd_rank[kTreeNodeCap], nd_lo[kTreeNodeCap], nd_hi[kTreeNodeCap];
  int list[kTreeNodeCap];  // the good islands of tree_make_children, then the stack of tree_leaves
  int nnodes, status, ngood, nleaf;
  int leaf_node[kTreeLeafCap];
  unsigned long long lf_key[kTreeLeafCap];
  int lf_area[kTreeLeafCap], lf_py[kTreeLeafCap], lf_px[kTreeLeafCap];
  double lf_s2[kTreeLeafCap];
};

__device__ __forceinline__ long long tree_q(float v) { return (long long)rint((double)v * kTreeFix); }

// 8-connected islands of {p : L[p] == node and snr[p] > lev}: lab[p] = the island's first pixel in raster order
// (kTreeNone outside the set).  Returns the number of islands (0 or 1 without labelling when the set has < 2 pixels).
__device__ int tree_islands(unsigned node, float lev, const TreeBox &B, TreeShared &S) {
  const int bw = B.bw, bh = B.bh, np = bw * bh, tid = threadIdx.x;
  uint16_t *lab = B.lab;
  int cnt = 0;
  for (int p = tid; p < np; p += kTreeThreads) {
    const bool m = B.L[p] == node && B.snr[p] > lev;
    lab[p] = m ? (uint16_t)p : (uint16_t)kTreeNone;
    cnt += m;
  }
  const int members = block_sum<kTreeWaves>(cnt, S.redi);
  if (members == 0) return 0;
  bool converged = members == 1;
  for (int sweep = 0; sweep < np && !converged; ++sweep) {
    int changed = 0;
    for (int p = tid; p < np; p += kTreeThreads) {
      const unsigned l = lab[p];
      if (l == kTreeNone) continue;
      const int i = p / bw, j = p - i * bw;
      unsigned m = l;
      // Two or three labels: a pair in one read, then the third.  That is the form hipcc gave this loop while it stood in
      // segment.hip; from this header it takes four lanes, which never run, and segment_kernel was 5 % slower at 64^2
      // (13.37 against 12.71 ms for 4000 stamps).  The pragma pins the earlier form.
      for (int y = max(i - 1, 0); y <= min(i + 1, bh - 1); ++y)
#pragma clang loop vectorize_width(2) interleave_count(1)
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
  for (int p = tid; p < np; p += kTreeThreads)
    if (lab[p] == p) {
      B.acc[p] = 0;
      ++cnt;
    }
  return block_sum<kTreeWaves>(cnt, S.redi);
}

// The islands labelled in lab become child nodes of `parent` where they pass the criterion of the node kind.
// kGroups (parent < 0): the groups of a stamp; an island of at least minarea pixels is good, one suffices, and nthresh
// and cont are handed down unchanged.  Otherwise a branch: flux above the parent's level >= cont * total, a split needs
// two, the children get half the levels and their share of the bar.
// Returns the number of children made (0: nothing changed).  Sets status 1 when the work list is full.
template <bool kGroups>
__device__ int tree_make_children(int parent, float lev, long long qt, long long total, double cont, int nthresh,
                                  int minarea, const TreeBox &B, TreeShared &S) {
  const int np = B.bw * B.bh, tid = threadIdx.x;
  const uint16_t *lab = B.lab;
  long long *acc = B.acc;
  if (tid == 0) S.ngood = 0;
  for (int p = tid; p < np; p += kTreeThreads) {
    const unsigned l = lab[p];
    if (l == kTreeNone) continue;
    const long long v = kGroups ? 1 : tree_q(B.snr[p]) - qt;
    atomicAdd((unsigned long long *)&acc[l], (unsigned long long)v);
  }
  __syncthreads();
  const double bar = cont * (double)total;
  for (int p = tid; p < np; p += kTreeThreads) {
    if (lab[p] != p) continue;
    const long long f = acc[p];
    const bool good = kGroups ? f >= (long long)minarea : (double)f >= bar;
    int slot = kTreeNodeCap;
    if (good) slot = atomicAdd(&S.ngood, 1);
    if (slot < kTreeNodeCap)
      S.list[slot] = p;
    else
      acc[p] = -1;
  }
  __syncthreads();
  const int ngood = S.ngood, base = S.nnodes;
  if (ngood < (kGroups ? 1 : 2)) return 0;
  if (base + ngood > kTreeNodeCap) {
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
    S.nd_nthresh[id] = kGroups ? nthresh : max(nthresh / 2, 4);
    S.nd_cont[id] = kGroups ? cont : (f > 0 ? bar / (double)f : 0.0);
    S.nd_first[id] = 0;
    S.nd_nchild[id] = 0;
    S.nd_parent[id] = parent;
    acc[p] = id;
  }
  __syncthreads();
  for (int p = tid; p < np; p += kTreeThreads) {
    const unsigned l = lab[p];
    if (l == kTreeNone) continue;
    const long long c = acc[l];
    if (c >= 0) B.L[p] = (uint8_t)c;
  }
  if (tid == 0) {
    if (!kGroups) {
      S.nd_first[parent] = base;
      S.nd_nchild[parent] = ngood;
    }
    S.nnodes = base + ngood;
  }
  __syncthreads();
  return ngood;
}

// The work list: every node in creation order, the ones it makes included, split at the first of its levels that has
// two good islands.  The caller has made the first nodes (nd_*, nnodes, L) and set status 0.
__device__ void tree_walk(const TreeBox &B, TreeShared &S) {
  const int np = B.bw * B.bh, tid = threadIdx.x;
  for (int x = 0; S.status == 0 && x < S.nnodes; ++x) {
    long long sq = 0;
    int ar = 0;
    unsigned pk = 0;
    for (int p = tid; p < np; p += kTreeThreads)
      if (B.L[p] == x) {
        sq += tree_q(B.snr[p]);
        ++ar;
        pk = max(pk, __float_as_uint(B.snr[p]));
      }
    const long long s0 = block_sum<kTreeWaves>(sq, S.red64);
    const int area = block_sum<kTreeWaves>(ar, S.redi);
    const float peak = __uint_as_float(block_max<kTreeWaves>(pk, S.redu));
    const float th = S.nd_thresh[x];
    const int nt = S.nd_nthresh[x];
    const double cont = S.nd_cont[x];
    const long long qt = tree_q(th);
    const long long total = s0 - (long long)area * qt;
    if (!(peak > th) || total <= 0) continue;
    float r = peak / th;
    for (int h = nt; h > 1; h >>= 1) r = sqrtf(r);
    float lev = th;
    for (int level = 1; level < nt; ++level) {
      lev = lev * r;
      const int kk = tree_islands((unsigned)x, lev, B, S);
      if (S.status != 0) break;
      if (kk < 2) continue;
      const int made = tree_make_children<false>(x, lev, qt, total, cont, nt, 0, B, S);
      if (made > 0 || S.status != 0) break;
    }
  }
}

// After the walk: the leaves numbered in depth-first order from every root (nd_rank, leaf_node, nleaf; status 1 above
// kTreeLeafCap), then the pixels a split left over go to a leaf under it, from the last node to the first (every
// descendant has a larger number).  Does nothing unless status is 0 and there is a node.
__device__ void tree_leaves(const TreeBox &B, TreeShared &S) {
  const int bw = B.bw, np = bw * B.bh, tid = threadIdx.x;
  if (S.status != 0 || S.nnodes == 0) return;
  if (tid == 0) {
    const int nn = S.nnodes;
    int *stack = S.list, sp = 0, nleaf = 0;  // the list is free by now; a node is pushed once, so kTreeNodeCap holds them
    for (int x = nn - 1; x >= 0; --x)
      if (S.nd_parent[x] < 0) stack[sp++] = x;
    while (sp > 0) {
      const int x = stack[--sp];
      if (S.nd_nchild[x] == 0) {
        S.nd_rank[x] = nleaf;
        if (nleaf < kTreeLeafCap) S.leaf_node[nleaf] = x;
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
    if (nleaf > kTreeLeafCap) S.status = 1;
  }
  __syncthreads();
  if (S.status != 0) return;
  for (int x = S.nnodes - 1; x >= 0; --x) {
    if (S.nd_nchild[x] == 0) continue;
    const int lo = S.nd_lo[x], hi = S.nd_hi[x];
    if (tid <= hi - lo) {
      S.lf_key[lo + tid] = 0;
      S.lf_area[lo + tid] = 0;
    }
    __syncthreads();
    for (int p = tid; p < np; p += kTreeThreads) {
      const unsigned node = B.L[p];
      if (node == kTreeNoNode || S.nd_nchild[node] != 0) continue;
      const int rk = S.nd_rank[node];
      if (rk < lo || rk > hi) continue;
      atomicAdd(&S.lf_area[rk], 1);
      // the largest snr, its first raster position
      atomicMax(&S.lf_key[rk],
                ((unsigned long long)__float_as_uint(B.snr[p]) << 32) | (0xFFFFFFFFu - (unsigned)p));
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
    for (int p = tid; p < np; p += kTreeThreads) {
      if (B.L[p] != x) continue;
      const int i = p / bw, j = p - i * bw;
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
      B.L[p] = (uint8_t)S.leaf_node[best];
    }
    __syncthreads();
  }
}

}  // namespace lc
