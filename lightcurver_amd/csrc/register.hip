// Registration of source lists by star triangles (DESIGN.md §5 "Frame registration"): astroalign.find_transform for K
// problems in one call, one workgroup per problem.
//
// The reference registers one frame at a time on the host (lightcurver/processes/alternate_plate_solving_adapt_existing_
// wcs.py:24, alternate_plate_solving_with_gaia.py:66: astroalign's KD-tree, itertools.combinations, a quadratic list
// de-duplication and a serial RANSAC).  Here a problem's points, triangles and invariants lie in LDS:
//   register_count_kernel   triangles of both lists, then the number of matching triangle pairs -> counts[k]
//   (the host waits once, sizes the table of matches by a prefix sum over the problems)
//   register_solve_kernel   the triangles again, the matches written at their exact offsets (two uint16 triangle indices
//                           each), the consensus in match order in chunks of one hypothesis per thread, the refits, the pairs
// Every comparison the SPEC makes is made on the same float64 bits (no fused multiply-adds; sqrt and division are correctly
// rounded); the sums of a fit are taken in a fixed order that depends on the problem alone: thread t adds the matches t,
// t + 256, ... in order, then a binary tree over the threads.  Nothing depends on K or on the other problems of the call.
#include <cmath>
#include <cstring>
#include <vector>

#include "device_call.h"
#include "lc_common.h"
#include "../../include/lcmi.h"

#pragma clang fp contract(off)  // the SPEC fixes every rounding: no fused multiply-adds, on the device or the host

namespace lc {

constexpr int kRegThreads = 256;
constexpr int kRegMinPoints = 3, kRegMaxPoints = 128;
constexpr int kRegNeighbours = 5;     // astroalign's NUM_NEAREST_NEIGHBORS
constexpr int kRegTriPerPoint = 10;   // C(5, 3)
constexpr int kRegScratchBytes = 4 * kRegThreads * (int)sizeof(double) + 2 * kRegMaxPoints * 8;

struct RegisterArgs {
  int P;
  const double *src, *tgt;        // [K][P][2]
  const int32_t *nsrc, *ntgt;     // [K]
  int32_t max_matches;
  double pixel_tol, radius, fraction;
  int32_t *counts;                // [K][3]: source triangles, target triangles, matches
  const int64_t *offset;          // [K]: the first record of problem k in matches (solve only)
  uint32_t *matches;              // source triangle | target triangle << 16
  double *transform;              // [K][6]
  int32_t *pairs;                 // [K][P][2] nullable
  int32_t *npairs, *diag, *status;  // [K], [K][5] nullable, [K]
};

// the LDS of one workgroup: points, triangles, and a region that holds the de-duplication's keys, then the invariants,
// then (once the matches are written) the scratch of the reductions
struct RegisterLds {
  double2 *pts[2];
  uchar4 *verts[2];   // a, b, c, keep
  double2 *inv[2];
  char *scratch;      // = inv[0]
  int *scan;          // [kRegThreads]
};

__host__ __device__ inline size_t register_lds_bytes(int P) {
  const size_t tri = (size_t)2 * kRegTriPerPoint * P;
  const size_t invb = tri * sizeof(double2);
  return (size_t)2 * P * sizeof(double2) + tri * sizeof(uchar4) + kRegThreads * sizeof(int) +
         (invb > (size_t)kRegScratchBytes ? invb : (size_t)kRegScratchBytes);
}

__device__ inline RegisterLds register_carve(char *smem, int P) {
  RegisterLds L;
  const int T = kRegTriPerPoint * P;
  L.pts[0] = reinterpret_cast<double2 *>(smem);
  L.pts[1] = L.pts[0] + P;
  L.verts[0] = reinterpret_cast<uchar4 *>(L.pts[1] + P);      // 32 P bytes in: 16-byte aligned
  L.verts[1] = L.verts[0] + T;
  L.scan = reinterpret_cast<int *>(L.verts[1] + T);           // 80 P bytes further
  L.inv[0] = reinterpret_cast<double2 *>(L.scan + kRegThreads);
  L.inv[1] = L.inv[0] + T;
  L.scratch = reinterpret_cast<char *>(L.inv[0]);
  return L;
}

__device__ inline double dist2(double2 p, double2 q) {
  const double dx = p.x - q.x, dy = p.y - q.y;
  return dx * dx + dy * dy;
}

// exclusive prefix sum of one int per thread (Hillis-Steele over `buf`, 256 ints); *total = the sum.  Barriers inside.
__device__ inline int block_scan(int v, int *buf, int *total) {
  const int t = threadIdx.x;
  __syncthreads();
  buf[t] = v;
  __syncthreads();
  for (int step = 1; step < kRegThreads; step <<= 1) {
    const int add = t >= step ? buf[t - step] : 0;
    __syncthreads();
    buf[t] += add;
    __syncthreads();
  }
  const int incl = buf[t];
  *total = buf[kRegThreads - 1];
  __syncthreads();
  return incl - v;
}

// Step 1 of the SPEC for one list: verts[0 .. T) and inv[0 .. T) of the surviving triangles in their order; returns T.
// `inv` holds the keys of the de-duplication before it takes the invariants.
__device__ int build_triangles(const double2 *pts, int n, uchar4 *verts, double2 *inv, int *scan) {
  const int tid = threadIdx.x;
  const int k = n < kRegNeighbours ? n : kRegNeighbours;
  const int per = k == 5 ? 10 : (k == 4 ? 4 : 1);
  const int traw = n * per;
  uint32_t *keys = reinterpret_cast<uint32_t *>(inv);                 // [traw]
  if (tid < n) {
    const double2 me = pts[tid];
    double bd[kRegNeighbours];
    int bi[kRegNeighbours];
#pragma unroll
    for (int q = 0; q < kRegNeighbours; ++q) {
      bd[q] = 0.0;
      bi[q] = -1;
    }
    for (int j = 0; j < n; ++j) {           // ascending j and a strict <: ties keep the lower index first
      const double d2 = dist2(pts[j], me);
#pragma unroll
      for (int q = kRegNeighbours - 1; q >= 0; --q) {
        if (bi[q] < 0 || d2 < bd[q]) {
          if (q < kRegNeighbours - 1) {
            bd[q + 1] = bd[q];
            bi[q + 1] = bi[q];
          }
          bd[q] = d2;
          bi[q] = j;
        }
      }
    }
    int slot = tid * per;
#pragma unroll
    for (int u = 0; u < kRegNeighbours; ++u)
#pragma unroll
      for (int v = u + 1; v < kRegNeighbours; ++v)
#pragma unroll
        for (int w = v + 1; w < kRegNeighbours; ++w) {
          if (w < k) {
            const int i0 = bi[u], i1 = bi[v], i2 = bi[w];
            const double s0 = sqrt(dist2(pts[i0], pts[i1])), s1 = sqrt(dist2(pts[i1], pts[i2])),
                         s2 = sqrt(dist2(pts[i0], pts[i2]));
            // ranks of a stable ascending sort of (s0, s1, s2)
            const int r0 = (s1 < s0) + (s2 < s0), r1 = (s0 <= s1) + (s2 < s1), r2 = (s0 <= s2) + (s1 <= s2);
            // the vertex a side does not touch: s0 -> i2, s1 -> i0, s2 -> i1; a faces L3, b faces L1, c faces L2
            const int a = r0 == 2 ? i2 : (r1 == 2 ? i0 : i1);
            const int b = r0 == 0 ? i2 : (r1 == 0 ? i0 : i1);
            const int c = r0 == 1 ? i2 : (r1 == 1 ? i0 : i1);
            const double l1 = r0 == 0 ? s0 : (r1 == 0 ? s1 : s2);
            const bool keep = l1 > 0.0;
            const int lo = min(i0, min(i1, i2)), hi = max(i0, max(i1, i2)), mid = i0 + i1 + i2 - lo - hi;
            verts[slot] = make_uchar4((unsigned char)a, (unsigned char)b, (unsigned char)c, keep ? 1 : 0);
            keys[slot] = (uint32_t)lo | ((uint32_t)mid << 8) | ((uint32_t)hi << 16);
            ++slot;
          }
        }
  }
  __syncthreads();
  // dropped if a LATER triangle has the same vertex set (every lane reads the same key: a broadcast)
  for (int t = tid; t < traw; t += kRegThreads) {
    const uint32_t key = keys[t];
    bool later = false;
    for (int u = 0; u < traw; ++u) later |= (u > t) & (keys[u] == key);
    if (later) verts[t].w = 0;
  }
  __syncthreads();
  // the survivors keep their order: thread t holds the raw triangles [t c, (t + 1) c)
  const int c = (traw + kRegThreads - 1) / kRegThreads;   // <= 5
  uchar4 mine[5];
  int kept = 0;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const int t = tid * c + q;
    mine[q] = make_uchar4(0, 0, 0, 0);
    if (q < c && t < traw) mine[q] = verts[t];
    kept += mine[q].w;
  }
  int total;
  int at = block_scan(kept, scan, &total);
#pragma unroll
  for (int q = 0; q < 5; ++q)
    if (mine[q].w) verts[at++] = mine[q];
  __syncthreads();
  for (int t = tid; t < total; t += kRegThreads) {
    const uchar4 v = verts[t];
    const double2 pa = pts[v.x], pb = pts[v.y], pc = pts[v.z];
    const double ab = sqrt(dist2(pa, pb)), ac = sqrt(dist2(pa, pc)), bc = sqrt(dist2(pb, pc));   // L2, L1, L3
    inv[t] = make_double2(bc / ab, ab / ac);
  }
  __syncthreads();
  return total;
}

__device__ inline bool tri_match(double2 p, double2 q, double radius) {
  const double dx = p.x - q.x, dy = p.y - q.y;
  return sqrt(dx * dx + dy * dy) <= radius;
}

__device__ inline void load_points(const RegisterArgs &A, int k, const RegisterLds &L, int ns, int nt) {
  const double2 *s = reinterpret_cast<const double2 *>(A.src) + (size_t)k * A.P;
  const double2 *t = reinterpret_cast<const double2 *>(A.tgt) + (size_t)k * A.P;
  for (int i = threadIdx.x; i < ns; i += kRegThreads) L.pts[0][i] = s[i];
  for (int i = threadIdx.x; i < nt; i += kRegThreads) L.pts[1][i] = t[i];
  __syncthreads();
}

// the matches of the rows [r0, r1) of this thread, counted; with `out` also written from out[0] on, by i then j
__device__ inline int match_rows(const RegisterLds &L, int r0, int r1, int tt, double radius, uint32_t *out) {
  int n = 0;
  for (int i = r0; i < r1; ++i) {
    const double2 p = L.inv[0][i];
    for (int j = 0; j < tt; ++j)
      if (tri_match(p, L.inv[1][j], radius)) {
        if (out) out[n] = (uint32_t)i | ((uint32_t)j << 16);
        ++n;
      }
  }
  return n;
}

extern __shared__ __attribute__((aligned(16))) char register_smem[];

__global__ __launch_bounds__(kRegThreads) void register_count_kernel(RegisterArgs A) {
  const int k = blockIdx.x, tid = threadIdx.x;
  const int ns = A.nsrc[k], nt = A.ntgt[k];
  int32_t *counts = A.counts + 3 * (size_t)k;
  if (ns < kRegMinPoints || nt < kRegMinPoints) {
    if (tid < 3) counts[tid] = 0;
    return;
  }
  const RegisterLds L = register_carve(register_smem, A.P);
  load_points(A, k, L, ns, nt);
  const int ts = build_triangles(L.pts[0], ns, L.verts[0], L.inv[0], L.scan);
  const int tt = build_triangles(L.pts[1], nt, L.verts[1], L.inv[1], L.scan);
  const int c = (ts + kRegThreads - 1) / kRegThreads;
  const int r0 = min(tid * c, ts), r1 = min(r0 + c, ts);
  const int mine = match_rows(L, r0, r1, tt, A.radius, nullptr);
  int total;
  block_scan(mine, L.scan, &total);
  if (tid == 0) {
    counts[0] = ts;
    counts[1] = tt;
    counts[2] = total;
  }
}

// ---- the consensus ------------------------------------------------------------------------------------------------------

struct Similarity {
  double a, b, tx, ty;
  bool ok;
};

struct Problem {
  const double2 *S, *T;     // the points
  const uchar4 *vs, *vt;    // the triangles
  const uint32_t *rec;      // the matches
  int n;
  double tol;
};

__device__ inline double vertex_error(const Similarity &M, double2 s, double2 t) {
  const double ex = M.a * s.x - M.b * s.y + M.tx - t.x;
  const double ey = M.b * s.x + M.a * s.y + M.ty - t.y;
  return sqrt(ex * ex + ey * ey);
}

// the three pairs of match m
__device__ inline void match_points(const Problem &Q, int m, double2 s[3], double2 t[3]) {
  const uint32_t r = Q.rec[m];
  const uchar4 a = Q.vs[r & 0xffffu], b = Q.vt[r >> 16];
  s[0] = Q.S[a.x];
  s[1] = Q.S[a.y];
  s[2] = Q.S[a.z];
  t[0] = Q.T[b.x];
  t[1] = Q.T[b.y];
  t[2] = Q.T[b.z];
}

// the largest of the three errors of match m is < tol
__device__ inline bool match_inlier(const Problem &Q, const Similarity &M, int m) {
  double2 s[3], t[3];
  match_points(Q, m, s, t);
  const double e = fmax(fmax(vertex_error(M, s[0], t[0]), vertex_error(M, s[1], t[1])), vertex_error(M, s[2], t[2]));
  return e < Q.tol;
}

__device__ inline Similarity similarity_from_sums(double A, double B, double d, double msx, double msy, double mtx, double mty) {
  Similarity M;
  M.ok = d != 0.0;
  M.a = A / d;
  M.b = B / d;
  M.tx = mtx - (M.a * msx - M.b * msy);
  M.ty = mty - (M.b * msx + M.a * msy);
  return M;
}

// step 3 on the three pairs of match m, summed in their order
__device__ inline Similarity fit_match(const Problem &Q, int m) {
  double2 s[3], t[3];
  match_points(Q, m, s, t);
  const double msx = (s[0].x + s[1].x + s[2].x) / 3.0, msy = (s[0].y + s[1].y + s[2].y) / 3.0;
  const double mtx = (t[0].x + t[1].x + t[2].x) / 3.0, mty = (t[0].y + t[1].y + t[2].y) / 3.0;
  double A = 0.0, B = 0.0, d = 0.0;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double sx = s[q].x - msx, sy = s[q].y - msy, tx = t[q].x - mtx, ty = t[q].y - mty;
    const double ta = sx * tx + sy * ty, tb = sx * ty - sy * tx, td = sx * sx + sy * sy;
    A = q ? A + ta : ta;
    B = q ? B + tb : tb;
    d = q ? d + td : td;
  }
  return similarity_from_sums(A, B, d, msx, msy, mtx, mty);
}

// sums of four doubles per thread over the workgroup, in a fixed binary tree: red is [4][kRegThreads]; the sums come back
// in v[] on every thread.  Barriers inside.
__device__ inline void block_sum4(double v[4], double *red) {
  const int t = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) red[q * kRegThreads + t] = v[q];
  __syncthreads();
  for (int step = kRegThreads / 2; step > 0; step >>= 1) {
    if (t < step) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[q * kRegThreads + t] = red[q * kRegThreads + t] + red[q * kRegThreads + t + step];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = red[q * kRegThreads];
  __syncthreads();
}

// Step 3 on the pairs of the matches that are inliers of `sel`, plus the match `forced` whatever its error (-1: none).
// *count = the number of those matches.  Every thread returns the same bits.
__device__ Similarity fit_inliers(const Problem &Q, const Similarity &sel, int forced, double *red, int *scan, int *count) {
  const int tid = threadIdx.x;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  int mine = 0;
  for (int m = tid; m < Q.n; m += kRegThreads) {
    if (!(m == forced || match_inlier(Q, sel, m))) continue;
    double2 s[3], t[3];
    match_points(Q, m, s, t);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      v[0] = v[0] + s[q].x;
      v[1] = v[1] + s[q].y;
      v[2] = v[2] + t[q].x;
      v[3] = v[3] + t[q].y;
    }
    ++mine;
  }
  int total;
  block_scan(mine, scan, &total);
  *count = total;
  block_sum4(v, red);
  Similarity M;
  M.ok = false;
  M.a = M.b = M.tx = M.ty = 0.0;
  if (total == 0) return M;
  const double np = (double)(3 * total);
  const double msx = v[0] / np, msy = v[1] / np, mtx = v[2] / np, mty = v[3] / np;
  double w[4] = {0.0, 0.0, 0.0, 0.0};
  for (int m = tid; m < Q.n; m += kRegThreads) {
    if (!(m == forced || match_inlier(Q, sel, m))) continue;
    double2 s[3], t[3];
    match_points(Q, m, s, t);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double sx = s[q].x - msx, sy = s[q].y - msy, tx = t[q].x - mtx, ty = t[q].y - mty;
      w[0] = w[0] + (sx * tx + sy * ty);
      w[1] = w[1] + (sx * ty - sy * tx);
      w[2] = w[2] + (sx * sx + sy * sy);
    }
  }
  block_sum4(w, red);
  return similarity_from_sums(w[0], w[1], w[2], msx, msy, mtx, mty);
}

__global__ __launch_bounds__(kRegThreads) void register_solve_kernel(RegisterArgs A) {
  const int k = blockIdx.x, tid = threadIdx.x;
  const int ns = A.nsrc[k], nt = A.ntgt[k];
  const double nan = __builtin_nan("");
  // what a problem without a solution leaves
  for (int i = tid; i < 6; i += kRegThreads) A.transform[6 * (size_t)k + i] = nan;
  if (A.pairs)
    for (int i = tid; i < 2 * A.P; i += kRegThreads) A.pairs[2 * (size_t)k * A.P + i] = -1;
  int32_t *diag = A.diag ? A.diag + 5 * (size_t)k : nullptr;
  if (ns < kRegMinPoints || nt < kRegMinPoints) {
    if (tid == 0) {
      A.status[k] = 3;
      A.npairs[k] = 0;
      if (diag) diag[0] = diag[1] = diag[2] = diag[4] = 0, diag[3] = -1;
    }
    return;
  }
  const RegisterLds L = register_carve(register_smem, A.P);
  load_points(A, k, L, ns, nt);
  const int ts = build_triangles(L.pts[0], ns, L.verts[0], L.inv[0], L.scan);
  const int tt = build_triangles(L.pts[1], nt, L.verts[1], L.inv[1], L.scan);
  const int c = (ts + kRegThreads - 1) / kRegThreads;
  const int r0 = min(tid * c, ts), r1 = min(r0 + c, ts);
  const int mine = match_rows(L, r0, r1, tt, A.radius, nullptr);
  int n;
  const int at = block_scan(mine, L.scan, &n);
  // the table was sized from the count kernel's n: the same code on the same bits.  Anything else is a fault of the
  // device, and nothing is written past the problem's share.
  const bool sized = n == A.counts[3 * (size_t)k + 2];
  int status = n > A.max_matches ? 2 : (n == 0 || !sized ? 1 : 0);
  int winner = -1, n_final = 0, npairs = 0;
  Similarity cur;
  cur.ok = false;
  if (status == 0) {
    uint32_t *rec = A.matches + A.offset[k];
    match_rows(L, r0, r1, tt, A.radius, rec + at);
    __syncthreads();   // the records are visible to the workgroup; the invariants' region becomes the reductions' scratch
    double *red = reinterpret_cast<double *>(L.scratch);
    int *s_win = reinterpret_cast<int *>(red + 4 * kRegThreads);   // and 2 * kRegMaxPoints ints of the pairs behind it
    Problem Q;
    Q.S = L.pts[0];
    Q.T = L.pts[1];
    Q.vs = L.verts[0];
    Q.vt = L.verts[1];
    Q.rec = rec;
    Q.n = n;
    Q.tol = A.pixel_tol;
    Similarity prev;
    bool all = false;
    if ((ns == 3 || nt == 3) && n == 1) {
      // astroalign's special case: one match of a three-point list is fitted without a consensus
      cur = fit_match(Q, 0);
      prev = cur;
      all = true;
      winner = 0;
      n_final = 1;
    } else {
      const int min_matches = max(1, min(10, (int)(A.fraction * (double)n)));
      for (int base = 0; base < n && winner < 0; base += kRegThreads) {
        if (tid == 0) *s_win = 0x7fffffff;
        __syncthreads();
        const int h = base + tid;
        if (h < n) {
          const Similarity M = fit_match(Q, h);
          if (M.ok) {
            int others = 0;
            for (int m = 0; m < n && others < min_matches; ++m) others += (m != h && match_inlier(Q, M, m)) ? 1 : 0;
            if (others >= min_matches) atomicMin(s_win, h);   // a minimum: the order of the lanes cannot reach it
          }
        }
        __syncthreads();
        if (*s_win != 0x7fffffff) winner = *s_win;
        __syncthreads();
      }
      if (winner >= 0) {
        const Similarity M = fit_match(Q, winner);
        cur = fit_inliers(Q, M, winner, red, L.scan, &n_final);
        for (int it = 0; it < 3 && cur.ok; ++it) {
          prev = cur;
          cur = fit_inliers(Q, prev, -1, red, L.scan, &n_final);
        }
      }
    }
    if (!cur.ok) {
      status = 1;
    } else {
      // step 5: for every source vertex of a final inlier match the target vertex of the smallest error, then by s
      int best_t = -1;
      double best_e = 0.0;
      if (tid < ns) {
        for (int m = 0; m < n; ++m) {
          const uint32_t r = rec[m];
          const uchar4 a = Q.vs[r & 0xffffu];
          if (a.x != tid && a.y != tid && a.z != tid) continue;
          if (!(all || match_inlier(Q, prev, m))) continue;
          const uchar4 b = Q.vt[r >> 16];
          const int t = a.x == tid ? b.x : (a.y == tid ? b.y : b.z);
          const double e = vertex_error(cur, Q.S[tid], Q.T[t]);
          if (best_t < 0 || e < best_e || (e == best_e && t < best_t)) {
            best_e = e;
            best_t = t;
          }
        }
      }
      const int pos = block_scan(best_t >= 0 ? 1 : 0, L.scan, &npairs);
      if (best_t >= 0 && A.pairs) {
        A.pairs[2 * ((size_t)k * A.P + pos)] = tid;
        A.pairs[2 * ((size_t)k * A.P + pos) + 1] = best_t;
      }
    }
  }
  if (tid == 0) {
    const bool solved = status == 0;
    if (solved) {
      double *o = A.transform + 6 * (size_t)k;
      o[0] = cur.a;
      o[1] = -cur.b;
      o[2] = cur.tx;
      o[3] = cur.b;
      o[4] = cur.a;
      o[5] = cur.ty;
    }
    A.status[k] = status;
    A.npairs[k] = solved ? npairs : 0;
    if (diag) {
      diag[0] = ts;
      diag[1] = tt;
      diag[2] = n;
      diag[3] = solved ? winner : -1;
      diag[4] = solved ? n_final : 0;
    }
  }
}

static bool register_cfg_ok(const lc_register_cfg *c) {
  return c->max_matches >= 1 && std::isfinite(c->pixel_tol) && c->pixel_tol > 0 && std::isfinite(c->invariant_radius) &&
         c->invariant_radius > 0 && std::isfinite(c->min_matches_fraction) && c->min_matches_fraction > 0;
}

}  // namespace lc

using namespace lc;

extern "C" {

int lc_register_supported(int max_points) { return max_points >= kRegMinPoints && max_points <= kRegMaxPoints ? 1 : 0; }

int lc_register_sources(lc_ctx *ctx, int K, int P, const double *src, const int32_t *nsrc, const double *tgt,
                        const int32_t *ntgt, const lc_register_cfg *cfg, double *transform, int32_t *pairs, int32_t *npairs,
                        int32_t *diag, int32_t *status, float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  if (K < 1 || !src || !nsrc || !tgt || !ntgt || !cfg || !transform || !npairs || !status)
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_register_sources: invalid argument");
  if (!lc_register_supported(P)) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_register_sources: P must be 3 .. 128 points");
  if (!register_cfg_ok(cfg))
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_register_sources: max_matches, the tolerances and the fraction must be finite and > 0");
  for (int k = 0; k < K; ++k) {
    if (nsrc[k] < 0 || nsrc[k] > P || ntgt[k] < 0 || ntgt[k] > P)
      LC_FAIL(ctx, LC_ERR_INVALID, "lc_register_sources: a count outside 0 .. P");
    const double *s = src + 2 * (size_t)k * P, *t = tgt + 2 * (size_t)k * P;
    for (int i = 0; i < 2 * nsrc[k]; ++i)
      if (!std::isfinite(s[i])) LC_FAIL(ctx, LC_ERR_INVALID, "lc_register_sources: a source coordinate that is not finite");
    for (int i = 0; i < 2 * ntgt[k]; ++i)
      if (!std::isfinite(t[i])) LC_FAIL(ctx, LC_ERR_INVALID, "lc_register_sources: a target coordinate that is not finite");
  }
  LC_ENTER(ctx);
  DeviceCall call(ctx);
  RegisterArgs A;
  std::memset(&A, 0, sizeof(A));
  A.P = P;
  A.max_matches = cfg->max_matches;
  A.pixel_tol = cfg->pixel_tol;
  A.radius = cfg->invariant_radius;
  A.fraction = cfg->min_matches_fraction;
  const size_t KP = (size_t)K * P;
  LC_HIP(ctx, call.upload(src, 2 * KP, &A.src));
  LC_HIP(ctx, call.upload(tgt, 2 * KP, &A.tgt));
  LC_HIP(ctx, call.upload(nsrc, (size_t)K, &A.nsrc));
  LC_HIP(ctx, call.upload(ntgt, (size_t)K, &A.ntgt));
  LC_HIP(ctx, call.alloc(3 * (size_t)K, &A.counts));
  LC_HIP(ctx, call.result(transform, 6 * (size_t)K, &A.transform));
  LC_HIP(ctx, call.result(pairs, 2 * KP, &A.pairs));
  LC_HIP(ctx, call.result(npairs, (size_t)K, &A.npairs));
  LC_HIP(ctx, call.result(diag, 5 * (size_t)K, &A.diag));
  LC_HIP(ctx, call.result(status, (size_t)K, &A.status));
  const size_t lds = register_lds_bytes(P);
  LC_HIP(ctx, call.start());
  hipLaunchKernelGGL(register_count_kernel, dim3((unsigned)K), dim3(kRegThreads), lds, ctx->stream, A);
  LC_HIP(ctx, hipGetLastError());
  // the one wait of the call: the table of matches is sized from the counts (a problem over max_matches takes none)
  std::vector<int32_t> counts(3 * (size_t)K);
  LC_HIP(ctx, hipMemcpyAsync(counts.data(), A.counts, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  LC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<int64_t> offset((size_t)K);
  int64_t total = 0;
  for (int k = 0; k < K; ++k) {
    offset[k] = total;
    const int32_t n = counts[3 * (size_t)k + 2];
    if (n > 0 && n <= cfg->max_matches) total += n;
  }
  LC_HIP(ctx, call.upload((const int64_t *)offset.data(), (size_t)K, &A.offset));
  LC_HIP(ctx, call.alloc((size_t)std::max<int64_t>(total, 1), &A.matches));
  hipLaunchKernelGGL(register_solve_kernel, dim3((unsigned)K), dim3(kRegThreads), lds, ctx->stream, A);
  LC_HIP(ctx, hipGetLastError());
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

}  // extern "C"
