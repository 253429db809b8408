// Difference imaging: a reference image PSF-matched to each frame and subtracted, frozen as the SPEC of DESIGN.md §5
// "Difference imaging".  Per chunk of frames and per round (one plus clip_iters) on the context's stream:
//
//   gram      the normal equations of every (frame, region) in float64.  A workgroup takes every split-th tile of 16 x 32
//             pixels of its region.  The reference tile with its r-pixel halo, the background terms and the frame's
//             pixels go to LDS once, as doubles; the design vector of a pixel is an addressing pattern into them and is
//             never formed.  The right-hand side is one more column of the design, so U and b are one lower triangle of
//             P + 1 rows, cut into blocks of 4 x 4 entries.  A lane owns one block and keeps its 16 sums in registers: 8
//             LDS reads per 16 multiply-adds.  Where a workgroup has fewer than 129 blocks its lanes also split the
//             tile's pixels into S slices, folded in the order of the slices at the end.  Partial sums are per workgroup.
//   fold      the workgroups' partial sums added in the order of the workgroups into the dense (P + 1)^2 matrix
//   (host)    Cholesky in float64 per (frame, region); the coefficients rounded to float32 go back with the status words
//   subtract  M and D = T - M in float32 in the SPEC's order, one lane per pixel, the reference tile in LDS; per tile the
//             residual sums over the round's fit set, folded in a fixed tree
//   residual  the tiles' sums added per (frame, region): every lane a strided share in the order of the tiles, then the
//             64 shares in the order of the lanes
// No floating-point atomics anywhere; the only atomic is the integer count of the fit set.  Every kernel reads the
// region's status word and leaves at once for a region that has failed.
#pragma clang fp contract(off)  // the SPEC fixes every rounding; the Gram sums use fma() by name

#include <chrono>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "device_call.h"
#include "frames_state.h"
#include "lc_common.h"
#include "resample_device.h"
#include "../../include/lcmi.h"

namespace lc {

constexpr int kDiThreads = 256;
constexpr int kDiTH = 16, kDiTW = 32;          // the tile of both tile kernels
constexpr int kDiTilePix = kDiTH * kDiTW;
constexpr int kDiBlk = 4;                      // a lane's block of the triangle: 4 x 4 entries
constexpr int kDiMaxR = 7, kDiMaxRegions = 64;
constexpr int kDiSplit = 16;                   // workgroups per frame over all regions (at least one per region)
constexpr int kDiExtPlanes = 8;                // LDS planes beside the reference: six background terms, T, zeros
constexpr size_t kDiScratchBytes = (size_t)128 << 20;
constexpr int kDiMaxChunkRegions = 65535;      // gridDim.z

struct DiRes {
  double s2, sw;   // sum of D^2 and of D^2 / sigma^2 over the fit set
  int32_t n, pad;
};

struct DiGeom {
  int H, W, r, kw, NK, nbg, P, P1, PB, NBLK, gy, gx, G, split, max_tiles;
  size_t hw;
};

struct DiArgs {
  DiGeom g;
  int round;
  float n_sigma;
  const float *T;         // [kc][H][W]
  const float *R;         // [H][W]
  const uint8_t *rfin;    // [H][W]: every reference pixel of the footprint is finite
  const float *var;       // [kc][H][W] or null
  const uint8_t *mask;    // [kc][H][W] or null
  const float *sigma;     // [kc] or null
  float *D;               // [kc][H][W]: the previous round's on entry
  int32_t *status;        // [kc G]
  const DiRes *res_in;    // [kc G]: the previous round's
  DiRes *res;             // [kc G]
  DiRes *res_part;        // [kc G][max_tiles]
  const short2 *blocks;   // [NBLK]: block row and column
  double *partial;        // [kc G][split][NBLK][16]
  double *aug;            // [kc G][P1][P1]
  int32_t *n_used;        // [kc G]
  const float *coef;      // [kc G][NK + 6]
};

struct DiRegion {
  int i0, i1, j0, j1, ntx, ntiles;
};

__host__ __device__ inline DiRegion di_region(const DiGeom &g, int reg) {
  const int gi = reg / g.gx, gj = reg % g.gx;
  DiRegion q;
  q.i0 = (int)((int64_t)gi * g.H / g.gy);
  q.i1 = (int)((int64_t)(gi + 1) * g.H / g.gy);
  q.j0 = (int)((int64_t)gj * g.W / g.gx);
  q.j1 = (int)((int64_t)(gj + 1) * g.W / g.gx);
  q.ntx = (q.j1 - q.j0 + kDiTW - 1) / kDiTW;
  q.ntiles = q.ntx * ((q.i1 - q.i0 + kDiTH - 1) / kDiTH);
  return q;
}

// the region's coordinate of row or column i of [i0, i1), in double
__device__ __forceinline__ double di_coord(int i, int i0, int i1) {
  const int span = i1 - i0 - 1;
  return (double)(2 * (int64_t)i - ((int64_t)i0 + i1 - 1)) / (double)(span > 1 ? span : 1);
}

// sigma of pixel p of frame k (chunk-local): sqrt(var), sigma[k], or the previous round's rms
__device__ __forceinline__ float di_sigma(const DiArgs &A, int k, int kg, size_t p) {
  if (A.var) return sqrtf(A.var[(size_t)k * A.g.hw + p]);
  if (A.sigma) return A.sigma[k];
  const DiRes q = A.res_in[kg];
  return (float)sqrt(q.s2 / (double)q.n);
}

// the fit set of the round: the weight of the pixel, 0 outside the set
__device__ __forceinline__ double di_weight(const DiArgs &A, int k, int kg, int i, int j) {
  const DiGeom &g = A.g;
  if (i < g.r || i >= g.H - g.r || j < g.r || j >= g.W - g.r) return 0.0;
  const size_t p = (size_t)i * g.W + j, kp = (size_t)k * g.hw + p;
  if (!A.rfin[p] || !__builtin_isfinite(A.T[kp])) return 0.0;
  if (A.mask && A.mask[kp]) return 0.0;
  double w = 1.0;
  if (A.var) {
    const float v = A.var[kp];
    if (!__builtin_isfinite(v) || !(v > 0.0f)) return 0.0;
    w = 1.0 / (double)v;
  }
  if (A.round > 0 && !(fabsf(A.D[kp]) <= A.n_sigma * di_sigma(A, k, kg, p))) return 0.0;
  return w;
}

// every reference pixel of the footprint of (i, j) is finite; 0 within r pixels of the border
__global__ __launch_bounds__(kDiThreads) void di_footprint_kernel(int H, int W, int r, const float *R, uint8_t *rfin) {
  const size_t p = (size_t)blockIdx.x * kDiThreads + threadIdx.x;
  if (p >= (size_t)H * W) return;
  const int i = (int)(p / W), j = (int)(p % W);
  bool ok = i >= r && i < H - r && j >= r && j < W - r;
  if (ok)
    for (int v = -r; v <= r; ++v)
      for (int u = -r; u <= r; ++u) ok = ok && __builtin_isfinite(R[(size_t)(i + v) * W + (j + u)]);
  rfin[p] = ok ? 1 : 0;
}

struct DiWarpArgs {
  int n, H, W, h, w, order, x0, y0;
  const float *planes;
  const int32_t *frame;   // [n] of the chunk
  const double *affine;   // [n][6]
  const float *scale;     // [n]: float32(|det A|)
  float *T;               // [n][H][W]
};

// the resample of the co-add, one lane per (frame of the chunk, pixel)
__global__ __launch_bounds__(kDiThreads) void di_warp_kernel(DiWarpArgs A) {
  const size_t hw = (size_t)A.H * A.W;
  const size_t p = (size_t)blockIdx.x * kDiThreads + threadIdx.x;
  const int k = blockIdx.y;
  if (p >= hw) return;
  const int i = (int)(p / A.W), j = (int)(p % A.W);
  A.T[(size_t)k * hw + p] = co_resample(A.planes + (size_t)A.frame[k] * A.h * A.w, A.h, A.w, A.affine + (size_t)k * 6,
                                        (double)(A.x0 + j), (double)(A.y0 + i), A.order, A.scale[k]);
}

// LDS offset of design entry m relative to the pixel's own offset li * PW + lj
__device__ __forceinline__ int di_offset(const DiGeom &g, int m, int PW, int ext0) {
  if (m < g.NK) return (2 * g.r - m / g.kw) * PW + (2 * g.r - m % g.kw);
  const int q = m - g.NK;
  const int plane = q < g.nbg ? q : (q == g.nbg ? 6 : 7);
  return ext0 + plane * kDiTH * PW;
}

__global__ __launch_bounds__(kDiThreads) void di_gram_kernel(DiArgs A) {
  extern __shared__ __align__(16) double di_lds[];
  const DiGeom &g = A.g;
  const int kg = blockIdx.z, k = kg / g.G, reg = kg % g.G;
  const int chunk = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  if (A.status[kg] != 0) return;
  const DiRegion q = di_region(g, reg);
  const int PW = kDiTW + 2 * g.r, PH = kDiTH + 2 * g.r;
  const int ext0 = PH * PW;
  double *ext = di_lds + ext0;
  double *wt = ext + kDiExtPlanes * kDiTH * PW;
  const int nb = min(kDiThreads, g.NBLK - chunk * kDiThreads);
  const int S = kDiThreads / nb;
  const int b = tid % nb, sl = tid / nb;
  const bool active = sl < S;
  const short2 blk = A.blocks[chunk * kDiThreads + b];
  int offm[kDiBlk], offn[kDiBlk];
#pragma unroll
  for (int e = 0; e < kDiBlk; ++e) {
    offm[e] = di_offset(g, blk.x * kDiBlk + e, PW, ext0);
    offn[e] = di_offset(g, blk.y * kDiBlk + e, PW, ext0);
  }
  double acc[kDiBlk][kDiBlk];
#pragma unroll
  for (int a = 0; a < kDiBlk; ++a)
#pragma unroll
    for (int c = 0; c < kDiBlk; ++c) acc[a][c] = 0.0;
  int count = 0;
  for (int t = s; t < q.ntiles; t += g.split) {
    const int ti0 = q.i0 + (t / q.ntx) * kDiTH, tj0 = q.j0 + (t % q.ntx) * kDiTW;
    __syncthreads();
    for (int idx = tid; idx < PH * PW; idx += kDiThreads) {
      const int i = ti0 - g.r + idx / PW, j = tj0 - g.r + idx % PW;
      di_lds[idx] = (i >= 0 && i < g.H && j >= 0 && j < g.W) ? (double)A.R[(size_t)i * g.W + j] : 0.0;
    }
    for (int idx = tid; idx < kDiTilePix; idx += kDiThreads) {
      const int li = idx / kDiTW, lj = idx % kDiTW;
      const int i = ti0 + li, j = tj0 + lj;
      double w = 0.0;
      if (i < q.i1 && j < q.j1) w = di_weight(A, k, kg, i, j);
      wt[idx] = w;
      const int o = li * PW + lj;
      double tv = 0.0, X = 0.0, Y = 0.0;
      if (w != 0.0) {
        tv = (double)A.T[(size_t)k * g.hw + (size_t)i * g.W + j];
        X = di_coord(j, q.j0, q.j1);
        Y = di_coord(i, q.i0, q.i1);
        ++count;
      }
      ext[0 * kDiTH * PW + o] = 1.0;
      ext[1 * kDiTH * PW + o] = X;
      ext[2 * kDiTH * PW + o] = Y;
      ext[3 * kDiTH * PW + o] = X * X;
      ext[4 * kDiTH * PW + o] = X * Y;
      ext[5 * kDiTH * PW + o] = Y * Y;
      ext[6 * kDiTH * PW + o] = tv;
      ext[7 * kDiTH * PW + o] = 0.0;
    }
    __syncthreads();
    if (active) {
      for (int p = sl; p < kDiTilePix; p += S) {
        const double w = wt[p];
        if (w == 0.0) continue;
        const double *px = di_lds + (p / kDiTW) * PW + (p % kDiTW);
        double am[kDiBlk], an[kDiBlk];
#pragma unroll
        for (int e = 0; e < kDiBlk; ++e) {
          am[e] = w * px[offm[e]];
          an[e] = px[offn[e]];
        }
#pragma unroll
        for (int a = 0; a < kDiBlk; ++a)
#pragma unroll
          for (int c = 0; c < kDiBlk; ++c) acc[a][c] = fma(am[a], an[c], acc[a][c]);
      }
    }
  }
  if (chunk == 0 && count) atomicAdd(A.n_used + kg, count);
  // the slices' sums in the order of the slices
  __syncthreads();
  if (active) {
#pragma unroll
    for (int a = 0; a < kDiBlk; ++a)
#pragma unroll
      for (int c = 0; c < kDiBlk; ++c) di_lds[((size_t)sl * nb + b) * 16 + a * kDiBlk + c] = acc[a][c];
  }
  __syncthreads();
  double *out = A.partial + (((size_t)kg * g.split + s) * g.NBLK + (size_t)chunk * kDiThreads) * 16;
  for (int idx = tid; idx < nb * 16; idx += kDiThreads) {
    double v = 0.0;
    for (int x = 0; x < S; ++x) v = v + di_lds[(size_t)x * nb * 16 + idx];
    out[idx] = v;
  }
}

// the workgroups' partial sums in the order of the workgroups, into the dense symmetric matrix
__global__ __launch_bounds__(kDiThreads) void di_fold_kernel(DiArgs A) {
  const DiGeom &g = A.g;
  const int kg = blockIdx.y;
  const int idx = blockIdx.x * kDiThreads + threadIdx.x;
  if (A.status[kg] != 0 || idx >= g.NBLK * 16) return;
  const short2 blk = A.blocks[idx / 16];
  const int e = idx % 16;
  const int row = blk.x * kDiBlk + e / kDiBlk, col = blk.y * kDiBlk + e % kDiBlk;
  if (row >= g.P1 || col > row) return;
  const double *p = A.partial + (size_t)kg * g.split * g.NBLK * 16 + idx;
  double v = 0.0;
  for (int s = 0; s < g.split; ++s) v = v + p[(size_t)s * g.NBLK * 16];
  double *aug = A.aug + (size_t)kg * g.P1 * g.P1;
  aug[(size_t)row * g.P1 + col] = v;
  aug[(size_t)col * g.P1 + row] = v;
}

__global__ __launch_bounds__(kDiThreads) void di_subtract_kernel(DiArgs A) {
  extern __shared__ __align__(16) double di_lds[];
  const DiGeom &g = A.g;
  const int kg = blockIdx.z, k = kg / g.G, reg = kg % g.G;
  const int t = blockIdx.x, tid = threadIdx.x;
  const DiRegion q = di_region(g, reg);
  if (t >= q.ntiles) return;
  const bool failed = A.status[kg] != 0;
  const int PW = kDiTW + 2 * g.r, PH = kDiTH + 2 * g.r;
  // LDS: three doubles and an int per lane for the sums, then the coefficients and the reference tile as floats
  double *r_s2 = di_lds, *r_sw = di_lds + kDiThreads;
  int *r_n = (int *)(di_lds + 2 * kDiThreads);
  float *cf = (float *)(di_lds + 3 * kDiThreads);
  float *tile = cf + g.NK + 6;
  const int ti0 = q.i0 + (t / q.ntx) * kDiTH, tj0 = q.j0 + (t % q.ntx) * kDiTW;
  if (!failed) {
    for (int idx = tid; idx < g.NK + 6; idx += kDiThreads) cf[idx] = A.coef[(size_t)kg * (g.NK + 6) + idx];
    for (int idx = tid; idx < PH * PW; idx += kDiThreads) {
      const int i = ti0 - g.r + idx / PW, j = tj0 - g.r + idx % PW;
      tile[idx] = (i >= 0 && i < g.H && j >= 0 && j < g.W) ? A.R[(size_t)i * g.W + j] : 0.0f;
    }
  }
  __syncthreads();
  double s2 = 0.0, sw = 0.0;
  int n = 0;
  for (int idx = tid; idx < kDiTilePix; idx += kDiThreads) {
    const int li = idx / kDiTW, lj = idx % kDiTW;
    const int i = ti0 + li, j = tj0 + lj;
    if (i >= q.i1 || j >= q.j1) continue;
    const size_t p = (size_t)i * g.W + j, kp = (size_t)k * g.hw + p;
    float d = __builtin_nanf("");
    if (!failed) {
      const double w = di_weight(A, k, kg, i, j);   // reads the previous round's D before this round's is written
      const float tv = A.T[kp];
      if (A.rfin[p] && __builtin_isfinite(tv)) {
        float m = 0.0f;
        const float *px = tile + li * PW + lj;
        for (int a = 0; a < g.kw; ++a)
          for (int c = 0; c < g.kw; ++c) m = m + cf[a * g.kw + c] * px[(2 * g.r - a) * PW + (2 * g.r - c)];
        const float X = (float)di_coord(j, q.j0, q.j1), Y = (float)di_coord(i, q.i0, q.i1);
        float bgv = cf[g.NK];
        if (g.nbg >= 3) {
          bgv = bgv + cf[g.NK + 1] * X;
          bgv = bgv + cf[g.NK + 2] * Y;
        }
        if (g.nbg >= 6) {
          bgv = bgv + cf[g.NK + 3] * (X * X);
          bgv = bgv + cf[g.NK + 4] * (X * Y);
          bgv = bgv + cf[g.NK + 5] * (Y * Y);
        }
        m = m + bgv;
        d = tv - m;
        if (w != 0.0) {
          const double d2 = (double)d * (double)d;
          double sg2 = 1.0;
          if (A.var)
            sg2 = (double)A.var[kp];
          else if (A.sigma)
            sg2 = (double)A.sigma[k] * (double)A.sigma[k];
          ++n;
          s2 = s2 + d2;
          sw = sw + d2 / sg2;
        }
      }
    }
    A.D[kp] = d;
  }
  if (failed) return;
  r_s2[tid] = s2;
  r_sw[tid] = sw;
  r_n[tid] = n;
  __syncthreads();
  for (int step = kDiThreads / 2; step > 0; step >>= 1) {
    if (tid < step) {
      r_s2[tid] = r_s2[tid] + r_s2[tid + step];
      r_sw[tid] = r_sw[tid] + r_sw[tid + step];
      r_n[tid] = r_n[tid] + r_n[tid + step];
    }
    __syncthreads();
  }
  if (tid == 0) {
    DiRes o;
    o.s2 = r_s2[0];
    o.sw = r_sw[0];
    o.n = r_n[0];
    o.pad = 0;
    A.res_part[(size_t)kg * g.max_tiles + t] = o;
  }
}

// one wave per (frame, region)
__global__ __launch_bounds__(kWave) void di_residual_kernel(DiArgs A) {
  __shared__ double l_s2[kWave], l_sw[kWave];
  __shared__ int l_n[kWave];
  const DiGeom &g = A.g;
  const int kg = blockIdx.x, lane = threadIdx.x;
  const DiRegion q = di_region(g, kg % g.G);
  const bool failed = A.status[kg] != 0;
  double s2 = 0.0, sw = 0.0;
  int n = 0;
  if (!failed)
    for (int t = lane; t < q.ntiles; t += kWave) {
      const DiRes o = A.res_part[(size_t)kg * g.max_tiles + t];
      s2 = s2 + o.s2;
      sw = sw + o.sw;
      n = n + o.n;
    }
  l_s2[lane] = s2;
  l_sw[lane] = sw;
  l_n[lane] = n;
  __syncthreads();
  if (lane == 0) {
    DiRes o;
    o.s2 = 0.0;
    o.sw = 0.0;
    o.n = 0;
    o.pad = 0;
    for (int x = 0; x < kWave; ++x) {
      o.s2 = o.s2 + l_s2[x];
      o.sw = o.sw + l_sw[x];
      o.n = o.n + l_n[x];
    }
    A.res[kg] = o;
  }
}

// Cholesky of the P x P normal equations in place (lower triangle) and the solve; 0, or 2 at a pivot that is not positive
static int di_solve(int P, int P1, const double *aug, std::vector<double> &L, double *x) {
  L.assign((size_t)P * P, 0.0);
  for (int i = 0; i < P; ++i) {
    for (int j = 0; j <= i; ++j) {
      double s = aug[(size_t)i * P1 + j];
      const double *li = &L[(size_t)i * P], *lj = &L[(size_t)j * P];
      for (int c = 0; c < j; ++c) s -= li[c] * lj[c];
      if (i == j) {
        if (!(s > 0.0) || !std::isfinite(s)) return 2;
        L[(size_t)i * P + i] = std::sqrt(s);
      } else {
        L[(size_t)i * P + j] = s / lj[j];
      }
    }
  }
  for (int i = 0; i < P; ++i) {
    double s = aug[(size_t)P * P1 + i];
    for (int c = 0; c < i; ++c) s -= L[(size_t)i * P + c] * x[c];
    x[i] = s / L[(size_t)i * P + i];
  }
  for (int i = P - 1; i >= 0; --i) {
    double s = x[i];
    for (int c = i + 1; c < P; ++c) s -= L[(size_t)c * P + i] * x[c];
    x[i] = s / L[(size_t)i * P + i];
  }
  for (int i = 0; i < P; ++i)
    if (!std::isfinite(x[i])) return 2;
  return 0;
}

static int di_host_threads(int work_items) {
  int t = (int)std::thread::hardware_concurrency();
  if (t <= 0) t = 4;
  return std::max(1, std::min({t, 16, work_items}));
}

static bool di_geom(int h, int w, const lc_diffim_cfg *cfg, DiGeom *g) {
  if (!lc_diffim_supported(h, w, cfg->r, cfg->bg_degree, cfg->gy, cfg->gx)) return false;
  std::memset(g, 0, sizeof(*g));
  g->H = h;
  g->W = w;
  g->hw = (size_t)h * w;
  g->r = cfg->r;
  g->kw = 2 * cfg->r + 1;
  g->NK = g->kw * g->kw;
  g->nbg = cfg->bg_degree == 0 ? 1 : (cfg->bg_degree == 1 ? 3 : 6);
  g->P = g->NK + g->nbg;
  g->P1 = g->P + 1;
  g->PB = (g->P1 + kDiBlk - 1) / kDiBlk;
  g->NBLK = g->PB * (g->PB + 1) / 2;
  g->gy = cfg->gy;
  g->gx = cfg->gx;
  g->G = cfg->gy * cfg->gx;
  g->split = std::max(1, kDiSplit / g->G);
  for (int reg = 0; reg < g->G; ++reg) g->max_tiles = std::max(g->max_tiles, di_region(*g, reg).ntiles);
  return true;
}

static size_t di_gram_lds(const DiGeom &g) {
  const int PW = kDiTW + 2 * g.r, PH = kDiTH + 2 * g.r;
  const size_t tile = ((size_t)PH * PW + (size_t)kDiExtPlanes * kDiTH * PW + kDiTilePix) * sizeof(double);
  return std::max(tile, (size_t)kDiThreads * 16 * sizeof(double));
}

static size_t di_subtract_lds(const DiGeom &g) {
  const int PW = kDiTW + 2 * g.r, PH = kDiTH + 2 * g.r;
  return (size_t)3 * kDiThreads * sizeof(double) + ((size_t)g.NK + 6 + (size_t)PH * PW) * sizeof(float);
}

// device bytes per frame of a chunk beyond the inputs and the outputs
static size_t di_frame_bytes(const DiGeom &g, bool own_T, bool own_D) {
  size_t b = (size_t)g.G * ((size_t)g.split * g.NBLK * 16 * sizeof(double) + (size_t)g.P1 * g.P1 * sizeof(double) +
                            (size_t)g.max_tiles * sizeof(DiRes) + ((size_t)g.NK + 6) * sizeof(float) + 64);
  if (own_T) b += g.hw * sizeof(float);
  if (own_D) b += g.hw * sizeof(float);
  return b;
}

struct DiInputs {
  int n;                   // frames of the call
  const float *d_T;        // [n][H][W] on the device, or null: resampled per chunk from the set below
  const float *d_R;
  const float *d_var;      // [n][H][W] or null
  const uint8_t *d_mask;   // [n][H][W] or null
  const float *d_sigma;    // [n] or null
  // the frames form
  const lc_frames *set = nullptr;
  const int32_t *d_frame = nullptr;
  const double *d_affine = nullptr;
  const float *d_scale = nullptr;
  int order = 0, x0 = 0, y0 = 0;
};

// everything after the argument checks: both entry points
static int di_run(lc_ctx *ctx, DeviceCall &call, const DiGeom &g, const lc_diffim_cfg *cfg, const DiInputs &in, int chunk,
                  const lc_diffim_out *out, float *kernel_ms) {
  const int n = in.n, G = g.G, P = g.P, P1 = g.P1, NK = g.NK;
  DiArgs A;
  std::memset(&A, 0, sizeof(A));
  A.g = g;
  A.n_sigma = cfg->n_sigma;
  A.R = in.d_R;
  // the table of blocks, row-major over the lower triangle
  std::vector<short2> blocks((size_t)g.NBLK);
  {
    size_t e = 0;
    for (int bm = 0; bm < g.PB; ++bm)
      for (int bn = 0; bn <= bm; ++bn) blocks[e++] = make_short2((short)bm, (short)bn);
  }
  const short2 *d_blocks = nullptr;
  LC_HIP(ctx, call.upload((const short2 *)blocks.data(), blocks.size(), &d_blocks));
  A.blocks = d_blocks;
  uint8_t *d_rfin = nullptr;
  LC_HIP(ctx, call.alloc(g.hw, &d_rfin));
  A.rfin = d_rfin;
  float *d_diff = nullptr, *d_Tc = nullptr, *d_Dc = nullptr, *d_coef = nullptr;
  LC_HIP(ctx, call.result(out->diff, (size_t)n * g.hw, &d_diff));
  if (!in.d_T) LC_HIP(ctx, call.alloc((size_t)chunk * g.hw, &d_Tc));
  if (!d_diff) LC_HIP(ctx, call.alloc((size_t)chunk * g.hw, &d_Dc));
  const size_t cG = (size_t)chunk * G;
  double *d_partial = nullptr, *d_aug = nullptr;
  int32_t *d_status = nullptr, *d_nused = nullptr;
  DiRes *d_res = nullptr, *d_part = nullptr;
  LC_HIP(ctx, call.alloc(cG * g.split * g.NBLK * 16, &d_partial));
  LC_HIP(ctx, call.alloc(cG * P1 * P1, &d_aug));
  LC_HIP(ctx, call.alloc(cG, &d_status));
  LC_HIP(ctx, call.alloc(cG, &d_nused));
  LC_HIP(ctx, call.alloc(cG, &d_res));
  LC_HIP(ctx, call.alloc(cG * g.max_tiles, &d_part));
  LC_HIP(ctx, call.alloc(cG * (NK + 6), &d_coef));
  A.partial = d_partial;
  A.aug = d_aug;
  A.status = d_status;
  A.n_used = d_nused;
  A.res = d_res;
  A.res_in = d_res;
  A.res_part = d_part;
  A.coef = d_coef;
  const size_t gram_lds = di_gram_lds(g), sub_lds = di_subtract_lds(g);
  LC_HIP(ctx, hipFuncSetAttribute((const void *)di_gram_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gram_lds));
  LC_HIP(ctx, hipFuncSetAttribute((const void *)di_subtract_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sub_lds));

  std::vector<double> aug(cG * P1 * P1);
  std::vector<float> coef(cG * (NK + 6));
  std::vector<int32_t> status(cG), nused(cG);
  std::vector<DiRes> res(cG);
  float gram_ms = 0.f, sub_ms = 0.f;
  double solve_ms = 0.0;
  auto timed = [&](float *into) -> hipError_t {   // between ev0 and ev1, after a synchronise
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return e;
    float ms = 0.f;
    e = hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    *into += ms;
    return e;
  };
  const int nchunks_e = (g.NBLK + kDiThreads - 1) / kDiThreads;
  const double nan = std::nan("");

  LC_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  hipLaunchKernelGGL(di_footprint_kernel, dim3((unsigned)((g.hw + kDiThreads - 1) / kDiThreads)), dim3(kDiThreads), 0,
                     ctx->stream, g.H, g.W, g.r, in.d_R, d_rfin);
  LC_HIP(ctx, hipGetLastError());
  LC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  LC_HIP(ctx, timed(&sub_ms));

  for (int k0 = 0; k0 < n; k0 += chunk) {
    const int kc = std::min(chunk, n - k0);
    const int kcG = kc * G;
    A.var = in.d_var ? in.d_var + (size_t)k0 * g.hw : nullptr;
    A.mask = in.d_mask ? in.d_mask + (size_t)k0 * g.hw : nullptr;
    A.sigma = in.d_sigma ? in.d_sigma + k0 : nullptr;
    A.D = d_diff ? d_diff + (size_t)k0 * g.hw : d_Dc;
    LC_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if (in.d_T) {
      A.T = in.d_T + (size_t)k0 * g.hw;
    } else {
      DiWarpArgs Wa;
      std::memset(&Wa, 0, sizeof(Wa));
      Wa.n = kc;
      Wa.H = g.H;
      Wa.W = g.W;
      Wa.h = in.set->h;
      Wa.w = in.set->w;
      Wa.order = in.order;
      Wa.x0 = in.x0;
      Wa.y0 = in.y0;
      Wa.planes = in.set->planes;
      Wa.frame = in.d_frame + k0;
      Wa.affine = in.d_affine + (size_t)k0 * 6;
      Wa.scale = in.d_scale + k0;
      Wa.T = d_Tc;
      hipLaunchKernelGGL(di_warp_kernel, dim3((unsigned)((g.hw + kDiThreads - 1) / kDiThreads), (unsigned)kc),
                         dim3(kDiThreads), 0, ctx->stream, Wa);
      LC_HIP(ctx, hipGetLastError());
      A.T = d_Tc;
    }
    LC_HIP(ctx, hipMemsetAsync(d_status, 0, (size_t)kcG * sizeof(int32_t), ctx->stream));
    LC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    LC_HIP(ctx, timed(&sub_ms));
    std::fill(status.begin(), status.end(), 0);
    std::fill(nused.begin(), nused.end(), 0);

    for (int round = 0; round <= cfg->clip_iters; ++round) {
      bool any = false;
      for (int kg = 0; kg < kcG; ++kg) any = any || status[kg] == 0;
      if (!any) break;   // every region of the chunk has failed: D is NaN already, nothing further is launched
      A.round = round;
      LC_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
      LC_HIP(ctx, hipMemsetAsync(d_nused, 0, (size_t)kcG * sizeof(int32_t), ctx->stream));
      hipLaunchKernelGGL(di_gram_kernel, dim3((unsigned)nchunks_e, (unsigned)g.split, (unsigned)kcG), dim3(kDiThreads),
                         gram_lds, ctx->stream, A);
      LC_HIP(ctx, hipGetLastError());
      hipLaunchKernelGGL(di_fold_kernel, dim3((unsigned)((g.NBLK * 16 + kDiThreads - 1) / kDiThreads), (unsigned)kcG),
                         dim3(kDiThreads), 0, ctx->stream, A);
      LC_HIP(ctx, hipGetLastError());
      LC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
      LC_HIP(ctx, hipMemcpyAsync(aug.data(), d_aug, (size_t)kcG * P1 * P1 * sizeof(double), hipMemcpyDeviceToHost,
                                 ctx->stream));
      std::vector<int32_t> cnt((size_t)kcG);
      LC_HIP(ctx, hipMemcpyAsync(cnt.data(), d_nused, (size_t)kcG * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
      LC_HIP(ctx, timed(&gram_ms));

      const auto t0 = std::chrono::steady_clock::now();
      // the regions are independent: up to 16 host threads take every nt-th one (the solve of a region is the same
      // sequential code whichever thread runs it)
      auto solve_one = [&](int kg, std::vector<double> &L, std::vector<double> &x) {
        nused[kg] = cnt[kg];
        const double *a = &aug[(size_t)kg * P1 * P1];
        float *c = &coef[(size_t)kg * (NK + 6)];
        const size_t okg = (size_t)k0 * G + kg;
        if (out->gram)
          for (int i = 0; i < P; ++i) std::memcpy(out->gram + (okg * P + i) * P, a + (size_t)i * P1, (size_t)P * sizeof(double));
        if (out->rhs) std::memcpy(out->rhs + okg * P, a + (size_t)P * P1, (size_t)P * sizeof(double));
        status[kg] = cnt[kg] < 2 * P ? 1 : di_solve(P, P1, a, L, x.data());
        const bool ok = status[kg] == 0;
        double sum = 0.0;
        for (int m = 0; m < NK; ++m) {
          c[m] = (float)x[m];
          sum += x[m];
          if (out->kernel) out->kernel[okg * NK + m] = ok ? x[m] : nan;
        }
        for (int b = 0; b < 6; ++b) {
          c[NK + b] = b < g.nbg ? (float)x[NK + b] : 0.0f;
          if (out->bg) out->bg[okg * 6 + b] = ok ? (b < g.nbg ? x[NK + b] : 0.0) : nan;
        }
        if (out->scale) out->scale[okg] = ok ? sum : nan;
      };
      const int nt = (double)kcG * P * P * P < 2e7 ? 1 : di_host_threads(kcG);
      auto worker = [&](int first) {
        std::vector<double> Lw, xw((size_t)P);
        for (int kg = first; kg < kcG; kg += nt)
          if (status[kg] == 0) solve_one(kg, Lw, xw);
      };
      if (nt == 1) {
        worker(0);
      } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < nt; ++t) pool.emplace_back(worker, t);
        for (std::thread &t : pool) t.join();
      }
      solve_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

      LC_HIP(ctx, hipMemcpyAsync(d_coef, coef.data(), (size_t)kcG * (NK + 6) * sizeof(float), hipMemcpyHostToDevice,
                                 ctx->stream));
      LC_HIP(ctx, hipMemcpyAsync(d_status, status.data(), (size_t)kcG * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
      LC_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
      hipLaunchKernelGGL(di_subtract_kernel, dim3((unsigned)g.max_tiles, 1, (unsigned)kcG), dim3(kDiThreads), sub_lds,
                         ctx->stream, A);
      LC_HIP(ctx, hipGetLastError());
      hipLaunchKernelGGL(di_residual_kernel, dim3((unsigned)kcG), dim3(kWave), 0, ctx->stream, A);
      LC_HIP(ctx, hipGetLastError());
      LC_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
      LC_HIP(ctx, timed(&sub_ms));   // (the copies above read host vectors that the next round rewrites)
    }
    LC_HIP(ctx, hipMemcpyAsync(res.data(), d_res, (size_t)kcG * sizeof(DiRes), hipMemcpyDeviceToHost, ctx->stream));
    LC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int kg = 0; kg < kcG; ++kg) {
      const size_t okg = (size_t)k0 * G + kg;
      if (out->status) out->status[okg] = status[kg];
      if (out->n_used) out->n_used[okg] = nused[kg];
      if (out->chi2) {
        double c2 = nan;
        if (status[kg] == 0) {
          const DiRes &q = res[kg];
          const double dof = (double)(q.n - P);
          c2 = (in.d_var || in.d_sigma) ? q.sw / dof : (q.sw / (q.s2 / (double)q.n)) / dof;
        }
        out->chi2[okg] = c2;
      }
    }
  }
  LC_HIP(ctx, call.finish(nullptr));
  if (kernel_ms) *kernel_ms = gram_ms + sub_ms;
  if (out->split_ms) {
    out->split_ms[0] = gram_ms;
    out->split_ms[1] = (float)solve_ms;
    out->split_ms[2] = sub_ms;
  }
  return LC_OK;
}

static bool di_any_output(const lc_diffim_out *o) {
  return o->diff || o->kernel || o->bg || o->scale || o->n_used || o->chi2 || o->status || o->gram || o->rhs;   // (split_ms alone is no output)
}

// the checks of cfg that both entry points share: 0, or the message
static const char *di_check_cfg(const lc_diffim_cfg *cfg) {
  if (cfg->r < 1 || cfg->r > kDiMaxR) return "r must lie in 1 .. 7";
  if (cfg->bg_degree < 0 || cfg->bg_degree > 2) return "bg_degree must be 0, 1 or 2";
  if (cfg->gy < 1 || cfg->gx < 1 || (int64_t)cfg->gy * cfg->gx > kDiMaxRegions) return "gy, gx >= 1 with gy gx <= 64";
  if (cfg->clip_iters < 0) return "clip_iters must be >= 0";
  if (!(cfg->n_sigma > 0.f) || !std::isfinite(cfg->n_sigma)) return "n_sigma must be positive and finite";
  return nullptr;
}

static int di_chunk(const DiGeom &g, int n, int scratch_frames, bool own_T, bool own_D) {
  int chunk = scratch_frames > 0 ? scratch_frames
                                 : (int)std::max<size_t>(1, kDiScratchBytes / di_frame_bytes(g, own_T, own_D));
  chunk = std::min(chunk, n);
  return std::max(1, std::min(chunk, kDiMaxChunkRegions / g.G));
}

}  // namespace lc

using namespace lc;

extern "C" {

int lc_diffim_supported(int h, int w, int r, int bg_degree, int gy, int gx) {
  if (r < 1 || r > kDiMaxR || bg_degree < 0 || bg_degree > 2) return 0;
  if (gy < 1 || gx < 1 || (int64_t)gy * gx > kDiMaxRegions) return 0;
  if (h < 2 * r + 1 || w < 2 * r + 1 || (int64_t)h * w >= ((int64_t)1 << 31)) return 0;
  if (gy > h || gx > w) return 0;   // a region without a pixel
  return 1;
}

int lc_diffim_frames(lc_ctx *ctx, int K, int h, int w, const float *target, const float *reference, const float *var,
                     const uint8_t *mask, const float *sigma, const lc_diffim_cfg *cfg, const lc_diffim_out *out,
                     float *kernel_ms) {
  if (!ctx) return LC_ERR_INVALID;
  if (K < 1 || !target || !reference || !cfg || !out) LC_FAIL(ctx, LC_ERR_INVALID, "lc_diffim_frames: invalid argument");
  if (!di_any_output(out)) LC_FAIL(ctx, LC_ERR_INVALID, "lc_diffim_frames: no output");
  if (const char *msg = di_check_cfg(cfg)) LC_FAIL(ctx, LC_ERR_INVALID, std::string("lc_diffim_frames: ") + msg);
  if (sigma)
    for (int k = 0; k < K; ++k)
      if (!std::isfinite(sigma[k]) || !(sigma[k] > 0.f))
        LC_FAIL(ctx, LC_ERR_INVALID, "lc_diffim_frames: a sigma that is not finite or not > 0");
  DiGeom g;
  if (!di_geom(h, w, cfg, &g))
    LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_diffim_frames: h, w >= 2 r + 1 with h w < 2^31 and a pixel in every region");
  LC_ENTER(ctx);
  DeviceCall call(ctx);
  DiInputs in;
  in.n = K;
  LC_HIP(ctx, call.upload(target, (size_t)K * g.hw, &in.d_T));
  LC_HIP(ctx, call.upload(reference, g.hw, &in.d_R));
  LC_HIP(ctx, call.upload(var, (size_t)K * g.hw, &in.d_var));
  LC_HIP(ctx, call.upload(mask, (size_t)K * g.hw, &in.d_mask));
  LC_HIP(ctx, call.upload(sigma, (size_t)K, &in.d_sigma));
  return di_run(ctx, call, g, cfg, in, di_chunk(g, K, 0, false, !out->diff), out, kernel_ms);
}

int lc_frames_subtract_reference(lc_frames *f, int n, const int32_t *frame, const double *affine, int H, int W, int x0,
                                 int y0, int order, const float *reference, const float *sigma, const uint8_t *mask,
                                 const lc_diffim_cfg *cfg, int scratch_frames, const lc_diffim_out *out, float *kernel_ms) {
  if (!f) return LC_ERR_INVALID;
  lc_ctx *ctx = f->ctx;
  if (n < 1 || !frame || !affine || !reference || !cfg || !out)
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_subtract_reference: invalid argument");
  if (!di_any_output(out)) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_subtract_reference: no output");
  if (const char *msg = di_check_cfg(cfg)) LC_FAIL(ctx, LC_ERR_INVALID, std::string("lc_frames_subtract_reference: ") + msg);
  if (order != 1 && order != 3) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_subtract_reference: order must be 1 or 3");
  if (scratch_frames < 0) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_subtract_reference: scratch_frames must be >= 0");
  if (H < 1 || W < 1) LC_FAIL(ctx, LC_ERR_UNSUPPORTED, "lc_frames_subtract_reference: H and W must be >= 1");
  if ((int64_t)x0 + W > INT32_MAX || (int64_t)y0 + H > INT32_MAX)
    LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_subtract_reference: the grid leaves the range of int");
  std::vector<float> scale((size_t)n);
  for (int k = 0; k < n; ++k) {
    if (frame[k] < 0 || frame[k] >= f->K)
      LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_subtract_reference: a frame index outside the set");
    const double *M = affine + (size_t)k * 6;
    for (int i = 0; i < 6; ++i)
      if (!std::isfinite(M[i])) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_subtract_reference: an affine entry that is not finite");
    const double det = M[0] * M[4] - M[1] * M[3];
    if (det == 0.0 || !std::isfinite(det))
      LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_subtract_reference: an affine without an inverse");
    scale[k] = (float)std::fabs(det);   // the co-add's factor at flux scale 1
    if (!std::isfinite(scale[k])) LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_subtract_reference: an affine without an inverse");
    if (sigma && (!std::isfinite(sigma[k]) || !(sigma[k] > 0.f)))
      LC_FAIL(ctx, LC_ERR_INVALID, "lc_frames_subtract_reference: a sigma that is not finite or not > 0");
  }
  DiGeom g;
  if (!di_geom(H, W, cfg, &g))
    LC_FAIL(ctx, LC_ERR_UNSUPPORTED,
            "lc_frames_subtract_reference: H, W >= 2 r + 1 with H W < 2^31 and a pixel in every region");
  LC_ENTER(ctx);
  DeviceCall call(ctx);
  DiInputs in;
  in.n = n;
  in.d_T = nullptr;
  in.d_var = nullptr;
  in.set = f;
  in.order = order;
  in.x0 = x0;
  in.y0 = y0;
  LC_HIP(ctx, call.upload(reference, g.hw, &in.d_R));
  LC_HIP(ctx, call.upload(mask, (size_t)n * g.hw, &in.d_mask));
  LC_HIP(ctx, call.upload(sigma, (size_t)n, &in.d_sigma));
  LC_HIP(ctx, call.upload(frame, (size_t)n, &in.d_frame));
  LC_HIP(ctx, call.upload(affine, (size_t)n * 6, &in.d_affine));
  LC_HIP(ctx, call.upload((const float *)scale.data(), (size_t)n, &in.d_scale));
  return di_run(ctx, call, g, cfg, in, di_chunk(g, n, scratch_frames, true, !out->diff), out, kernel_ms);
}

}  // extern "C"
